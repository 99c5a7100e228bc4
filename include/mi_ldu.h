/*
 * mi_ldu.h -- C ABI of the MI355X-native lduMatrix / fvMatrix compute engine.
 *
 * This is the drop-in boundary for the hot path of SimFlowCFD/RapidCFD-dev
 * (SURVEY.md section 8b).  The reference has no FFI: the path sits behind
 * OpenFOAM's run-time selection tables (lduMatrix::solver / preconditioner /
 * smoother, lduMatrix.H:141-185,297-341,438-460) and the lduMatrix member
 * functions.  A maintainer binds this ABI from a C++ shim that registers the
 * same run-time names (INTEGRATION.md shows the stub); the C++ host mirror of
 * those classes lives in rapidcfd-dev_amd/foam/.
 *
 * Conventions
 *   - scalar = double, label = int32_t (reference defaults: etc/bashrc:76,
 *     primitives/ints/label/label.H:57-66).
 *   - Pointers named *_dev are DEVICE pointers owned by the caller (the
 *     reference's gpuList<T> storage, gpuList.H:23-112); *_host are host
 *     pointers.  The engine never frees caller memory.
 *   - Vectors passed across this ABI are in the CALLER's cell/face order.
 *     The engine keeps its own tiled order internally; the
 *     *_engine entry points work on vectors already in engine order.
 *   - Every function returns MI_OK (0) or a negative error code; the message
 *     is available from mi_last_error().  The reference aborts the process
 *     instead (FatalError / CUDA_CALL, DeviceConfig.H:6-11); the shim turns a
 *     non-zero status into FatalError.
 *   - One context per GPU / per rank, not thread-safe (the reference is one
 *     host thread per MPI rank, argList.C:775-811).
 *   - There is no CPU fallback: every compute entry point needs a gfx950
 *     device and fails with MI_ERR_DEVICE otherwise.
 *
 * All paths in citations are relative to /root/reference/src/OpenFOAM/matrices/lduMatrix/
 * unless they start with src/.
 */
#ifndef MI_LDU_H
#define MI_LDU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi_ctx_s *mi_ctx_t;
typedef struct mi_addr_s *mi_addr_t;
typedef struct mi_matrix_s *mi_matrix_t;
typedef struct mi_gamg_s *mi_gamg_t;
typedef struct mi_patch_s *mi_patch_t;
typedef struct mi_comm_s *mi_comm_t;

enum {
    MI_OK = 0,
    MI_ERR_ARG = -1,
    MI_ERR_DEVICE = -2,   /* no gfx950 device / HIP failure */
    MI_ERR_ALLOC = -3,
    MI_ERR_STATE = -4,    /* e.g. coefficients not bound */
    MI_ERR_LIMIT = -5,    /* mesh exceeds a tile-format limit */
    MI_ERR_UNSUPPORTED = -6 /* a combination this build does not provide (stated where it can occur) */
};

/* preconditioner names of lduMatrix::preconditioner::New
 * (lduMatrix/lduMatrixPreconditioner.C:67-158).  DIC/DILU resolve to AINV in
 * the reference (preconditioners/DICPreconditioner/DICPreconditioner.C:42-58). */
enum { MI_PRECOND_NONE = 0, MI_PRECOND_DIAGONAL = 1, MI_PRECOND_AINV = 2 };

/* solverPerformance (src/OpenFOAM/matrices/LduMatrix/LduMatrix/SolverPerformance.H) */
typedef struct {
    double initialResidual;
    double finalResidual;
    double normFactor;
    int32_t nIterations;
    int32_t converged;
    int32_t singular;
    int32_t reserved;
} mi_solver_perf;

/* lduMatrix::solver::readControls (lduMatrix/lduMatrixSolver.C:167-173) */
typedef struct {
    double tolerance; /* default 1e-6 */
    double relTol;    /* default 0    */
    int32_t maxIter;  /* default 1000 */
    int32_t minIter;  /* default 0    */
} mi_solver_controls;

/* ---- context (replaces src/OpenFOAM/device/DeviceConfig.{H,C}, DeviceStream) ---- */
/* stream: a hipStream_t created by the caller (e.g. torch's current stream) or NULL
 * for the engine's own stream.  MI_PCG_BATCH (iterations per batch of the device-resident
 * Krylov loops, default 16) below 1 is taken as 1.                                  */
int mi_ctx_create(int device, void *hip_stream, mi_ctx_t *out);
int mi_ctx_destroy(mi_ctx_t ctx);
int mi_ctx_synchronize(mi_ctx_t ctx);
/* run-time switches of a context (the environment variable of the same meaning sets the value a new context starts with):
 *   "pcg_persist" 0 / 1          the persistent PCG kernel for matrices whose tiles fit the CUs' registers (MI_PCG_PERSIST)
 *   "pcg_fuse_rp" 0 / 1          PCG on one GPU: residual update of an iteration + direction update of the next as one
 *                                launch that keeps the preconditioned residual on the chip (MI_PCG_FUSE_RP; same bits)
 *   "pcg_fuse_test" 0..3         tests: workgroups of that launch leave its barrier at once (1: every third, 2: the first)
 *   "win_direct" 0 / 1 / 2       operators of attached matrices as ONE launch whose boundary tiles read the halo window
 *                                (MI_WIN_DIRECT; 2: also between ranks that share a device -- tests)
 *   "gamg_graph_attached" 0 / 1  hipGraph replay of the V-cycle of a decomposed case (MI_GAMG_GRAPH_ATTACHED)             */
int mi_ctx_set_option(mi_ctx_t ctx, const char *name, int32_t value);
/* which solver paths ran on this context (diagnostics, tests): launches of the persistent PCG kernel -- one per batch of
 * iterations -- on plain (MI_STAT_PERSIST_PCG) / communicator-attached (MI_STAT_PERSIST_DPCG) matrices; runs of the grid
 * barrier litmus that gates that kernel (MI_STAT_BARRIER_LITMUS); V-cycles of a decomposed case replayed as a hipGraph
 * (MI_STAT_GAMG_GRAPH_ATTACHED); launches of the fused residual / direction kernel of PCG (MI_STAT_PCG_FUSED_RP); batches of
 * PCG iterations that mi_pcg_solve replayed from a hipGraph (MI_STAT_PCG_GRAPH); solves of one PBiCG loop per call --
 * mi_pbicg_solve or mi_pbicg_solve_multi -- through the multi-vector solver (MI_STAT_PBICG_MULTI), through the device loop
 * pbicg_solve_device (MI_STAT_PBICG_DEVICE, once per component) and host-stepped (MI_STAT_PBICG_HOST_STEPPED); PBiCGStab solves
 * through the device loop (MI_STAT_PBICGSTAB_DEVICE) and host-stepped (MI_STAT_PBICGSTAB_HOST_STEPPED); PBiCGStab solves of either
 * loop that ended at the mid-iteration exit, converged on the residual of sA (MI_STAT_PBICGSTAB_MID_EXIT); tile launches that
 * took the persistent walk of MI_TILE_PERSIST, fewer workgroups than tiles (MI_STAT_TILE_PERSIST).  (The device loops
 * share one host frame in csrc/engine.hip -- stage_in, drive_batches, finish_device -- around the bodies they enqueue:
 * bicg_enqueue for pbicg_solve_device, stab_enqueue for pbicgstab_solve_device, the in-line body of mi_pbicg_solve_multi.) */
#define MI_STAT_PERSIST_PCG 0
#define MI_STAT_PERSIST_DPCG 1
#define MI_STAT_BARRIER_LITMUS 2
#define MI_STAT_GAMG_GRAPH_ATTACHED 3
#define MI_STAT_PCG_FUSED_RP 4
#define MI_STAT_PCG_GRAPH 5
#define MI_STAT_PBICG_MULTI 6
#define MI_STAT_PBICG_DEVICE 7
#define MI_STAT_PBICG_HOST_STEPPED 8
#define MI_STAT_PBICGSTAB_DEVICE 9
#define MI_STAT_PBICGSTAB_HOST_STEPPED 10
#define MI_STAT_PBICGSTAB_MID_EXIT 11
#define MI_STAT_TILE_PERSIST 12
int mi_ctx_stat(mi_ctx_t ctx, int32_t which, int64_t *out);
const char *mi_last_error(void);
/* 1 if a usable gfx950 device is visible to this process, else 0 */
int mi_device_available(void);

/* ---- addressing (replaces lduAddressing demand-driven tables,
 *      lduAddressing/lduAddressing.H:128-145, .C:169-344; K23 in SURVEY.md) ----
 * lower/upper: host mirrors of lowerAddr/upperAddr (fvMeshLduAddressing.H:165-181),
 *   faces in OpenFOAM upper-triangular order is NOT required, only lower<upper.
 * patches: coupled (processor) interfaces, patch p has patch_sizes[p] faces whose
 *   internal cells are patch_face_cells_host[p][...] (fvMeshLduAddressing.H:113-120).
 * Builds the tiled engine layout once per mesh.                                   */
int mi_addr_create(mi_ctx_t ctx, int32_t n_cells, int32_t n_faces,
                   const int32_t *lower_addr_host, const int32_t *upper_addr_host,
                   int32_t n_patches, const int32_t *patch_sizes,
                   const int32_t *const *patch_face_cells_host, mi_addr_t *out);
/* Same, with LOCAL coupled patches (cyclic, cyclicLduInterfaceField: lduAddressing/lduInterfaceFields/
 * cyclicLduInterfaceField, src/finiteVolume/fields/fvPatchFields/constraint/cyclic): patch_nbr_cells_host[p] != NULL
 * gives, face by face, the local cell on the other side of patch p (the neighbour patch's faceCells in matching
 * order); the update result[faceCells] -= coeffs*psi[nbrCells] then needs no exchange and every solver entry
 * point works on such a matrix.  NULL entries are processor patches (ext region).                              */
int mi_addr_create_coupled(mi_ctx_t ctx, int32_t n_cells, int32_t n_faces,
                           const int32_t *lower_addr_host, const int32_t *upper_addr_host,
                           int32_t n_patches, const int32_t *patch_sizes,
                           const int32_t *const *patch_face_cells_host,
                           const int32_t *const *patch_nbr_cells_host, mi_addr_t *out);
/* cyclicAMI patch (row f3; src/finiteVolume/fields/fvPatchFields/constraint/cyclicAMI/cyclicAMIFvPatchField.C:195-224,
 * src/meshTools/AMIInterpolation/GAMG/interfaceFields/cyclicAMIGAMGInterfaceField/cyclicAMIGAMGInterfaceField.C:97-130,
 * AMIInterpolation/AMIInterpolationF.H:62-105): `patch` -- created WITHOUT neighbour cells, i.e. with an ext region like a
 * processor patch -- takes its neighbour values from the cells of `nbr_patch` of the same addressing through the AMI
 * addressing and weights of its side (srcAddress/srcWeights on the owner patch, tgtAddress/tgtWeights on the other):
 *     pnf[i] = sum_{k in [start[i], start[i+1])} weights[k] * ( factor * psi[ faceCells(nbr_patch)[ address[k] ] ] )
 * one fused multiply-add per term in address order (multiplyWeightedOp<plusEqOp> under nvcc's contraction), factor =
 * mi_matrix_set_patch_transform; low_weight[i] != 0 (weightsSum[i] < lowWeightCorrection, decided by the caller) replaces
 * the sum by the face's own cell value, the default the reference passes (`pif`).  The two sides may differ in size.  Every
 * operator and solver that reads coupled-patch neighbour values interpolates them before its tile pass; no exchange.
 * start/address/weights all NULL: one face to one face with unit weight -- a cyclic (or processorCyclic-on-one-rank) patch
 * that needs its transformation factor (cyclicLduInterfaceField.C:45-62).
 * GAMG (mi_gamg_create on such an addressing; mergeLevels 1): every level carries the agglomerated AMI -- one coarse patch
 * face per distinct local coarse cell in order of first appearance (cyclicAMIGAMGInterface.C:47-165), addresses and
 * weights agglomerated with the face areas of mi_addr_set_ami_face_areas and renormalised (AMIInterpolation::agglomerate,
 * AMIInterpolation.C:279-540; no low-weight correction on coarse levels, :751).  The coarsest level is solved iteratively:
 * mi_gamg_solve wants directSolveCoarsest = 0 there, as the reference's direct coarsest solver casts every interface to a
 * cyclic one (LUscalarMatrix.C:246-251) and cannot run such a case either.                                               */
int mi_addr_set_ami_patch(mi_addr_t addr, int32_t patch, int32_t nbr_patch, const int32_t *start_host_or_null,
                          const int32_t *address_host_or_null, const double *weights_host_or_null,
                          const uint8_t *low_weight_host_or_null);
/* cyclicAMI whose PARTNER patch lives on another rank (round 4; the reference's distributed AMI: singlePatchProc_ == -1,
 * src/meshTools/AMIInterpolation/AMIInterpolation/AMIInterpolation.C:940-1091 calcProcMap + mapDistribute, :281-520 agglomerate
 * with targetMapPtr).  The partner's patch-internal field travels through an ordinary PROCESSOR patch of this addressing, the
 * transport patch: created like any processor patch (no neighbour cells), the SAME size on both ranks (the larger AMI side,
 * padded), its faceCells = this side's AMI faceCells (padding entries: any cell), its interface coefficients zero
 * (mi_matrix_set_interface_coeffs), so the matrix never sees it and every transport of the engine carries it as it is; in
 * mi_matrix_attach_comm it names the partner rank and the partner's transport patch.
 *     pnf[i] = sum_k weights[k] * ( factor * received[ address[k] ] ),  address[k] = face of the transport patch whose
 * received value is meant (finest level: the partner's face number; < n_partner_faces <= size of the transport patch).
 * The interpolation runs after the halo exchange of the operator (such a matrix exchanges first and runs all tiles in one
 * launch).  GAMG: as for a local cyclicAMI patch; the partner side's coarse faces follow from the coarse cells the transport
 * patch receives on every level, no further talk between the ranks.
 * mi_addr_set_ami_patch_remote_multi (round 6): the partner SIDE is itself split over several ranks -- what decomposePar makes of
 * any cyclicAMI patch larger than one rank's share; the reference: calcProcMap (AMIInterpolation.C:940-1091) builds a map that
 * brings every target face a rank's source faces overlap, from whichever rank holds it, into one list numbered rank by rank
 * (AMIInterpolationParallelOps.C).  Here: ONE transport patch per partner piece (as above, each between this rank and the rank
 * that holds the piece), and address[k] numbers the pieces' faces CONCATENATED in the order of transport_patches: piece q =
 * [n_partner_faces[0] + ... + n_partner_faces[q-1], + n_partner_faces[q]), its face j = face j of transport patch q.  A face's
 * weighted sum may take terms from several pieces; they are added in address order, as on one rank.  GAMG: every piece's coarse
 * faces are derived from what ITS transport patch receives, piece by piece (each rank agglomerates its own piece).          */
int mi_addr_set_ami_patch_remote(mi_addr_t addr, int32_t patch, int32_t transport_patch, int32_t n_partner_faces,
                                 const int32_t *start_host, const int32_t *address_host, const double *weights_host,
                                 const uint8_t *low_weight_host_or_null);
int mi_addr_set_ami_patch_remote_multi(mi_addr_t addr, int32_t patch, int32_t n_transports, const int32_t *transport_patches_host,
                                       const int32_t *n_partner_faces_host, const int32_t *start_host, const int32_t *address_host,
                                       const double *weights_host, const uint8_t *low_weight_host_or_null);
/* face areas |Sf| of a cyclicAMI patch's faces (AMIInterpolation::srcMagSf / tgtMagSf), read by the GAMG agglomeration only */
int mi_addr_set_ami_face_areas(mi_addr_t addr, int32_t patch, const double *mag_sf_host);
/* ORDERED addressing -- the caller's numbering is kept: engine order == caller order, mi_addr_cell_perm is the identity and the
 * caller-order operators (mi_amul, mi_tmul, mi_residual, mi_H, mi_sumA, mi_precondition, mi_jacobi_smooth) run straight on the
 * caller's arrays, with no permutation passes (only an n_cells copy of the input where an operator reads coupled-patch
 * neighbour values, which live behind the owned values of an engine vector).  This is how fields "live in engine order for
 * the life of the mesh": renumber the mesh ONCE with the cell order an ordinary mi_addr_create proposes (mi_addr_cell_perm =
 * new-to-old cell map, the `cellMap` renumberMesh's manual method reads; src/renumber/renumberMethods/manualRenumber), keep
 * mi_addr_tile_starts with it, and create the addressing of the renumbered mesh here.  tile_cell_start NULL: consecutive
 * cells are cut into tiles greedily (any numbering with locality, e.g. after a Cuthill-McKee renumberMesh).
 * lduAddressing itself is unchanged by this (lowerAddr/upperAddr of the renumbered mesh, upper-triangular as always).        */
int mi_addr_create_ordered(mi_ctx_t ctx, int32_t n_cells, int32_t n_faces, const int32_t *lower_host, const int32_t *upper_host,
                           int32_t n_patches, const int32_t *patch_sizes, const int32_t *const *patch_face_cells_host,
                           const int32_t *const *patch_nbr_cells_host_or_null, int32_t n_tiles, const int32_t *tile_cell_start_host_or_null,
                           mi_addr_t *out);
/* RENUMBER AT BIND (round 3): the two steps above as ONE call for a mesh that was never renumberMesh-ed -- the shim adopts the
 * engine's cell order for the life of the mesh.  Builds the clustered layout of the mesh as given, renumbers the cells into the
 * engine order and the faces into the upper-triangular order of that numbering (faces whose owner and neighbour swap are
 * flipped), and returns the ORDERED addressing of the renumbered mesh together with what polyMesh::renumber / mapPolyMesh need:
 *   cell_new_to_old [n_cells]   new cell i = old cell map[i]                 (the cellMap of renumberMesh's manual method)
 *   face_new_to_old [n_faces]   new internal face f = old face map[f]
 *   face_flipped    [n_faces]   1: its owner / neighbour (hence upper / lower, and the sign of a flux) swapped
 *   lower_out / upper_out       the addressing of the renumbered mesh (any of the five outputs may be NULL)
 * Fields are permuted ONCE when they are read (new[i] = old[cell_new_to_old[i]]) and back when they are written; from then on
 * every operator of this ABI runs on the caller's arrays without permutation passes (mi_amul 0.62-0.70 of the HBM roofline
 * instead of 0.52 through the permuting addressing).  Patch face cells (and local partner cells) are renumbered inside; their
 * face order is kept.  mi_layout_adopt_host: the host part alone (no device; tests).                                           */
int mi_addr_create_adopted(mi_ctx_t ctx, int32_t n_cells, int32_t n_faces, const int32_t *lower_host, const int32_t *upper_host,
                           int32_t n_patches, const int32_t *patch_sizes, const int32_t *const *patch_face_cells_host,
                           const int32_t *const *patch_nbr_cells_host_or_null, int32_t *cell_new_to_old_out, int32_t *face_new_to_old_out,
                           uint8_t *face_flipped_out, int32_t *lower_out, int32_t *upper_out, mi_addr_t *out);
int mi_layout_adopt_host(int32_t n_cells, int32_t n_faces, const int32_t *lower_host, const int32_t *upper_host, int32_t n_patches,
                         const int32_t *patch_sizes, const int32_t *const *patch_face_cells_host, const int32_t *const *patch_nbr_cells_host_or_null,
                         int32_t *cell_new_to_old_out, int32_t *face_new_to_old_out, uint8_t *face_flipped_out, int32_t *lower_out,
                         int32_t *upper_out, int32_t *n_tiles_out);
/* the tiles of a layout as ranges of ENGINE cells: n_tiles + 1 offsets (mi_addr_n_tiles) */
int mi_addr_tile_starts(mi_addr_t addr, int32_t *tile_cell_start_out_host);
/* 1 when engine order == caller order (mi_addr_create_ordered, or a numbering that happened to be tile-contiguous) */
int mi_addr_is_ordered(mi_addr_t addr);
int mi_addr_destroy(mi_addr_t addr);
int32_t mi_addr_n_cells(mi_addr_t addr);
int32_t mi_addr_n_faces(mi_addr_t addr);
int32_t mi_addr_n_tiles(mi_addr_t addr);
/* number of halo ("external") cells appended after the n_cells owned cells in
 * engine-order vectors: sum of patch sizes                                       */
int32_t mi_addr_n_ext(mi_addr_t addr);
/* engine->caller cell permutation (n_cells ints) */
int mi_addr_cell_perm(mi_addr_t addr, int32_t *engine_to_caller_host);
/* layout statistics: [0]=tiles [1]=slots total [2]=entries total (padded)
 * [3]=halo entries total [4]=max cells/tile [5]=max slots/tile [6]=max halo/tile
 * [7]=LDS bytes per workgroup (symmetric)                                        */
int mi_addr_stats(mi_addr_t addr, int64_t stats[8]);

/* ---- matrix (replaces lduMatrix storage + lowerSort()/upperSort() caches,
 *      lduMatrix/lduMatrix.C:221-472; K22 calcSortCoeffs) ---- */
int mi_matrix_create(mi_addr_t addr, mi_matrix_t *out);
mi_addr_t mi_matrix_addr(mi_matrix_t m);   /* the addressing a matrix was created on (borrowed handle) */
int mi_matrix_destroy(mi_matrix_t m);
/* Bind new coefficient values ("coefficients changed" epoch; the reference
 * invalidates lowerSortPtr_ in every mutator, lduMatrix.C:235,266).
 * lower_dev == NULL => symmetric (lower aliases upper, lduMatrix.C:328-345).
 * Copies into the engine's tiled layout; the caller arrays are not retained.    */
int mi_matrix_set_coeffs(mi_matrix_t m, const double *diag_dev, const double *upper_dev,
                         const double *lower_dev);
/* interfaceBouCoeffs / interfaceIntCoeffs of coupled patch p (device pointers,
 * patch_sizes[p] values each; int_coeffs_dev may be NULL for symmetric matrices). */
int mi_matrix_set_interface_coeffs(mi_matrix_t m, int32_t patch, const double *bou_coeffs_dev,
                                   const double *int_coeffs_dev);
/* transformCoupleField of a coupled patch (cyclicLduInterfaceField.C:45-62, processorGAMGInterfaceField.C:213,230,
 * cyclicAMILduInterfaceField.C:45-62): the neighbour values are multiplied by
 *     factor = pow(diag(forwardT).component(cmpt), rank)
 * before they enter result -= coeffs*pnf -- 1 for scalars (rank 0) and untransformed patches, the caller's number for the
 * component solves of a vector across a rotational cyclic / processorCyclic.  Processor patches: applied to the received
 * values; cyclicAMI and one-to-one patches declared with mi_addr_set_ami_patch: applied before the interpolation.  A plain
 * cyclic patch (created with neighbour cells) only accepts 1.  Held per matrix: Ux, Uy, Uz solves set their own.
 * Decomposed case: the FIRST factor of a matrix is set before mi_matrix_attach_comm -- the ranks agree there whether the case
 * has transformed patches anywhere (it decides the solver pipeline of EVERY rank); afterwards the values may change freely,
 * but a first factor != 1 on a case that was attached without any is refused (MI_ERR_STATE).                              */
int mi_matrix_set_patch_transform(mi_matrix_t m, int32_t patch, double factor);

/* ---- halo (replaces init/updateMatrixInterfaces + processorFvPatchField
 *      gather/scatter, lduMatrixUpdateMatrixInterfaces.C:30-276,
 *      src/finiteVolume/fields/fvPatchFields/constraint/processor/processorFvPatchScalarField.C:36-170) ----
 * pack: send_dev[patch_offset[p]+i] = x[patch_face_cells[p][i]] for all patches
 *       (K5 fvPatchTemplates.C:49-63), x in engine order.
 * The received neighbour values are written by the caller (RCCL recv / peer copy)
 * straight into the ext region x_engine[n_cells .. n_cells+n_ext).              */
int mi_halo_pack_engine(mi_addr_t addr, const double *x_engine_dev, double *send_dev);
int mi_addr_patch_offsets(mi_addr_t addr, int32_t *offsets_host /* n_patches+1 */);

/* ---- vector layout helpers ---- */
int mi_vec_to_engine(mi_addr_t addr, const double *x_caller_dev, double *x_engine_dev);
int mi_vec_from_engine(mi_addr_t addr, const double *x_engine_dev, double *x_caller_dev);

/* ---- SpMV family, caller order (lduMatrix::Amul/Tmul lduMatrixATmul.C:183-342,
 *      sumA :345-395, residual :397-496, H1 :533-554, H lduMatrixOperations.C:130-154,
 *      faceH lduMatrixTemplates.C:110-148) ----
 * Interface (halo) terms use ext values previously placed with mi_matrix_set_ext (single
 * process: none).  On an addressing that permutes (mi_addr_create) these run the tile pass straight on the caller's arrays:
 * x is gathered through the cell permutation while a tile is staged, y (and source) are addressed through it in the row
 * loop -- no separate permutation passes (mi_amul 173 us against 146 in engine order on the 216^3 box); with ordered
 * addressing there is no permutation at all.                                                                            */
int mi_amul(mi_matrix_t m, const double *psi_dev, double *Apsi_dev);
int mi_tmul(mi_matrix_t m, const double *psi_dev, double *Tpsi_dev);
int mi_sumA(mi_matrix_t m, double *sumA_dev);
int mi_residual(mi_matrix_t m, const double *psi_dev, const double *source_dev, double *rA_dev);
int mi_H(mi_matrix_t m, const double *psi_dev, double *H_dev);
int mi_H1(mi_matrix_t m, double *H1_dev);
int mi_faceH(mi_matrix_t m, const double *psi_dev, double *faceH_dev);
/* neighbour values for the coupled patches, caller patch order, n_ext doubles */
int mi_matrix_set_ext(mi_matrix_t m, const double *ext_values_dev);

/* ---- SpMV family, engine order (inner loops of the solvers; what bench.py times) ----
 * vectors are n_cells + n_ext long; which: 0 = all tiles, 1 = interior tiles only
 * (no ext reference), 2 = boundary tiles only (after the halo has arrived).       */
int mi_amul_engine(mi_matrix_t m, const double *psi_e, double *Apsi_e, int which);
int mi_tmul_engine(mi_matrix_t m, const double *psi_e, double *Tpsi_e, int which);

/* ---- engine-order primitives for a caller that keeps its own solver loop but lets its work vectors live in engine order for
 *      the duration of a solve (mi_vec_to_engine once, mi_vec_from_engine once): the same operators without the permutation
 *      passes of the caller-order entry points (measured on the 216^3 box: the reference's PCG::solve runs at 682 us/iteration
 *      on the caller-order primitives).  mi_amul_engine / mi_tmul_engine with which = 0 exchange the halo
 *      themselves when a communicator is attached; reductions (mi_sum*) do not care about the order.                      */
int mi_precondition_engine(mi_matrix_t m, int kind, int transpose, const double *rA_e, double *wA_e);
int mi_residual_engine(mi_matrix_t m, const double *psi_e, const double *source_e, double *rA_e);
int mi_jacobi_smooth_engine(mi_matrix_t m, double omega, double *psi_e, const double *source_e, int32_t n_sweeps);
int mi_norm_factor_engine(mi_matrix_t m, const double *psi_e, const double *source_e, const double *Apsi_e, double *out_host);

/* ---- preconditioners (lduMatrix::preconditioner::precondition / preconditionT,
 *      diagonalPreconditioner.C:45-89, AINVPreconditioner.C:49-120) ---- */
int mi_precondition(mi_matrix_t m, int kind, int transpose, const double *rA_dev, double *wA_dev);

/* ---- smoother (lduMatrix::smoother::smooth; JacobiSmoother.C:39-148; the
 *      reference's "GaussSeidel" is this Jacobi with omega 0.9) ---- */
int mi_jacobi_smooth(mi_matrix_t m, double omega, double *psi_dev, const double *source_dev,
                     int32_t n_sweeps);

/* ---- field reductions (gpuFieldCommonFunctions.C:351-367,420-440,492-511) ----
 * deterministic fixed-tree device reductions; result returned to the host.       */
int mi_sum(mi_ctx_t ctx, const double *a_dev, int64_t n, double *out_host);
int mi_sum_prod(mi_ctx_t ctx, const double *a_dev, const double *b_dev, int64_t n, double *out_host);
int mi_sum_mag(mi_ctx_t ctx, const double *a_dev, int64_t n, double *out_host);
/* lduMatrix::solver::normFactor (lduMatrixSolver.C:182-236):
 *   sum(|Apsi - avg(psi)*sumA| + |source - avg(psi)*sumA|) + small_ ; caller order; the same
 * bits as perf.normFactor of the whole solvers; global when a communicator is attached.  */
int mi_norm_factor(mi_matrix_t m, const double *psi_dev, const double *source_dev,
                   const double *Apsi_dev, double *out_host);

/* ---- whole solvers (lduMatrix::solver::solve; PCG.C:68-208, PBiCG.C:67-246,
 *      PBiCGStab.C:67-300, smoothSolver.C:77-196).  psi in/out, caller order.
 * residual_history_host (may be NULL) receives the normalised residual after
 * every iteration, [0] = initial; history_len entries at most.                    */
int mi_pcg_solve(mi_matrix_t m, double *psi_dev, const double *source_dev,
                 const mi_solver_controls *controls, int precond,
                 mi_solver_perf *perf_out, double *residual_history_host, int32_t history_len);
/* The same PCG as a session, for callers that want to overlap or time it
 * themselves (bench.py): begin = PCG.C:85-121 (A.psi, rA, normFactor, initial
 * residual); iterate = enqueue n_iters bodies of the do-loop (PCG.C:133-204) on
 * the context's stream WITHOUT synchronising -- bodies past convergence are
 * device-side no-ops, so the result equals the reference loop; end = fetch psi,
 * solverPerformance and the residual history.  If amul_ms_sum != NULL, every
 * Amul launch of this call is bracketed by HIP events on the stream and the sum
 * of their durations is returned (this synchronises).
 * One session per context: between mi_pcg_begin and mi_pcg_end the session owns the context's solver scratch
 * (device-side solver state, reduction partials) and the matrix's work vectors; until mi_pcg_end the reductions
 * (mi_sum*), mi_norm_factor*, every mi_*_solve and a mi_pcg_begin on another matrix of the same context return
 * MI_ERR_STATE instead of corrupting the running solve.  The operators (mi_amul ... mi_precondition) stay usable. */
int mi_pcg_begin(mi_matrix_t m, const double *psi0_dev, const double *source_dev,
                 const mi_solver_controls *controls, int precond, int32_t history_len);
int mi_pcg_iterate(mi_matrix_t m, int32_t n_iters, float *amul_ms_sum);
/* same, events around every event_stride-th Amul only; *amul_ms_sum = mean sampled duration x n_iters */
int mi_pcg_iterate_sampled(mi_matrix_t m, int32_t n_iters, int32_t event_stride, float *amul_ms_sum);
int mi_pcg_end(mi_matrix_t m, double *psi_out_dev, mi_solver_perf *perf_out,
               double *residual_history_host, int32_t history_len);

/* ---- GAMG (solvers/GAMG/GAMGSolver.C:47-249, GAMGSolverSolve.C:59-619, GAMGSolverScale.C:59-171,
 *      GAMGSolverAgglomerateMatrix.C:37-321, GAMGAgglomerations/.../pairGAMGAgglomerate.C:31-313,
 *      GAMGAgglomerateLduAddressing.C:245-461, GAMGAgglomerationTemplates.C:35-308) ----
 * mi_gamg_create builds the pair-agglomeration hierarchy once per mesh (host, cached like the
 * reference's GAMGAgglomeration MeshObject) and one engine layout per level.
 *   face_weights_host: [n_faces] agglomeration weights -- faceAreaPair passes
 *     |Sf/sqrt|Sf| o (1,1.01,1.02)| (src/finiteVolume/.../faceAreaPairGAMGAgglomeration.C:54-81),
 *     algebraicPair passes |upper|.
 *   n_cells_in_coarsest_level: the mandatory fvSolution key (GAMGAgglomeration.C:96-99).
 *   merge_levels: fvSolution's mergeLevels (pairGAMGAgglomerate.C:110-117): every level folds that many pair steps
 *     (GAMGAgglomeration::combineLevels, GAMGAgglomerateLduAddressing.C:606-760); 1 = one pair step per level.
 *   forward_init: the reference's process-wide static sweep direction (pairGAMGAgglomeration.C:33),
 *     true in a fresh process; mi_gamg_forward_out returns its value after the build.
 * mi_gamg_solve agglomerates the level matrices from the matrix's current coefficients (the
 * reference does this on every solver construction, GAMGSolver.C:88-97), then runs V-cycles.
 * Smoother: Jacobi omega (the reference's "GaussSeidel", JacobiSmoother.C:34-36).  The coarsest
 * level is solved directly (directSolveCoarsest, GAMGSolver.C:144-172) with a dense inverse kept
 * on the device.  scaleCorrection < 0 selects the reference default (= symmetric).            */
typedef struct {
    double tolerance, relTol;
    int32_t maxIter, minIter;
    int32_t nPreSweeps, preSweepsLevelMultiplier, maxPreSweeps;     /* 0, 1, 4 */
    int32_t nPostSweeps, postSweepsLevelMultiplier, maxPostSweeps;  /* 2, 1, 4 */
    int32_t nFinestSweeps, scaleCorrection;                         /* 2, -1   */
    double omega;                                                   /* 0.9     */
    int32_t directSolveCoarsest;  /* 1 (GAMGSolver.C:77): dense solve on the device; 0: ICCG / BICCG (PCG / PBiCG + AINV, */
    int32_t reserved;             /* GAMG's tolerance and relTol, zero start) on the coarsest level, GAMGSolverSolve.C:572-613 */
} mi_gamg_controls;
int mi_gamg_create(mi_addr_t fine_addr, const double *face_weights_host, int32_t n_cells_in_coarsest_level,
                   int32_t merge_levels, int forward_init, mi_gamg_t *out);
/* Same for a matrix with coupled patches.  Cyclic (local) patches need no communicator (pass NULLs; mi_gamg_create
 * does that).  Processor patches (processorGAMGInterface, solvers/GAMG/interfaces/processorGAMGInterface/
 * processorGAMGInterface.C:54-245; GAMGAgglomerateLduAddressing.C:464-520) need the communicators the matrix is
 * attached to: the ranks agree on when to stop (GAMGAgglomeration.C:72-81), exchange the restrict addressing of the
 * patch cells on every level, every level matrix exchanges its own halo, the scale factors are all-reduced
 * (GAMGSolverScale.C:104-107) and the coarsest level is the GLOBAL system (LUscalarMatrix.C:57-150) whose dense
 * inverse every rank holds the rows of.  All ranks call create/solve together.                                  */
/* agglomerator "dummy" (GAMGAgglomerations/dummyAgglomeration/dummyAgglomeration.C:45-90; the reference's debugging
 * agglomerator): n_levels levels whose restrict addressing is the identity -- every level is the fine mesh again, the
 * coarsest (= fine) system is solved directly, so it is for small meshes (<= 4096 cells with directSolveCoarsest). */
int mi_gamg_create_dummy(mi_addr_t fine_addr, int32_t n_levels, mi_gamg_t *out);
int mi_gamg_create_coupled(mi_addr_t fine_addr, const double *face_weights_host,
                           int32_t n_cells_in_coarsest_level, int32_t merge_levels, int forward_init, mi_comm_t reduce_or_null,
                           mi_comm_t halo_or_null, const int32_t *patch_rank,
                           const int32_t *patch_nbr_patch_or_null, mi_gamg_t *out);
int mi_gamg_destroy(mi_gamg_t g);
int32_t mi_gamg_n_levels(mi_gamg_t g);
int mi_gamg_forward_out(mi_gamg_t g);
/* out4 = {n_fine_cells, n_fine_faces, n_coarse_cells, n_coarse_faces} of coarse level `level` */
int mi_gamg_level_sizes(mi_gamg_t g, int32_t level, int32_t out4[4]);
int mi_gamg_solve(mi_gamg_t g, mi_matrix_t m, double *psi_dev, const double *source_dev,
                  const mi_gamg_controls *controls, mi_solver_perf *perf_out,
                  double *residual_history_host, int32_t history_len);
/* level operators in the caller order of each level (restrictField / prolongField,
 * GAMGAgglomerationTemplates.C:35-153,273-308) and the agglomerated level coefficients
 * (GAMGSolverAgglomerateMatrix.C:218-317); used by the parity tests                          */
int mi_gamg_restrict(mi_gamg_t g, int32_t level, const double *fine_dev, double *coarse_dev);
int mi_gamg_prolong(mi_gamg_t g, int32_t level, const double *coarse_dev, double *fine_dev);
/* The pieces of the V-cycle as operators, for a caller that keeps the reference's GAMGSolverSolve.C and swaps only the
 * primitives (tests/ref_dropin runs exactly that):
 *   mi_gamg_update        agglomerateMatrix of every level from the matrix's current coefficients + the coarsest direct
 *                         solver (the GAMGSolver constructor, GAMGSolver.C:88-172); mi_gamg_solve does it itself.
 *   mi_gamg_level_matrix  matrixLevels_[level] as a BORROWED handle (vectors in the hierarchy's coarse-cell numbering):
 *                         mi_amul / mi_jacobi_smooth / mi_residual ... work on it.
 *   mi_gamg_scale         GAMGSolver::scale (GAMGSolverScale.C:59-171) on the fine or a level matrix.
 *   mi_gamg_solve_coarsest  solveCoarsestLevel with directSolveCoarsest (GAMGSolverSolve.C:552-570), on the device.    */
int mi_gamg_update(mi_gamg_t g, mi_matrix_t m);
int mi_gamg_level_matrix(mi_gamg_t g, int32_t level, mi_matrix_t *level_matrix_out);
int mi_gamg_scale(mi_matrix_t m, double *field_dev, double *Acf_dev, const double *source_dev);
int mi_gamg_solve_coarsest(mi_gamg_t g, const double *source_dev, double *corr_dev);
int mi_gamg_level_coeffs(mi_gamg_t g, mi_matrix_t m, int32_t level, double *diag_out_dev,
                         double *upper_out_dev, double *lower_out_dev);

/* ---- fvMatrix assembly sweeps, scalar fields, caller-order device arrays ----
 * (src/finiteVolume/finiteVolume/convectionSchemes/gaussConvectionScheme/gaussConvectionScheme.C:74-115,
 *  .../laplacianSchemes/gaussLaplacianScheme/gaussLaplacianScheme.C:44-88,
 *  src/OpenFOAM/matrices/lduMatrix/lduMatrix/lduMatrixOperations.C:36-106,
 *  src/finiteVolume/fvMatrices/fvMatrix/fvMatrix.C:38-124,208-349,1087-1345,
 *  src/finiteVolume/finiteVolume/fvc/fvcSurfaceIntegrate.C:40-96,
 *  src/finiteVolume/interpolation/surfaceInterpolation/surfaceInterpolationScheme/surfaceInterpolationScheme.C:337-352)
 * Every scheme is one streaming face pass + one row pass whose own-face reads are staged through LDS
 * (the reference: 3-6 Thrust passes + temporaries).  They need the caller's faces owner-sorted
 * (OpenFOAM's upper-triangular order); face fields 16-byte aligned.
 * A mesh without internal faces (one cell; cells joined by patches only) is legal: every face array is
 * empty, its pointer may be NULL and is never read, every row sum is +0.0; mi_fvm_assemble* then takes
 * each face term as present and empty.
 * mi_row_face_op kind: 0 sumDiag, 1 negSumDiag, 2 sumMagOffDiag; lower_dev NULL => symmetric.
 * mi_patch_*: a boundary patch = its faceCells; mi_patch_add applies pf per unique cell in ascending
 * patch-face order (addToInternalField, K26): fn 0 add, 1 subtract, 2 add magnitudes.          */
int mi_row_face_op(mi_addr_t addr, int kind, const double *lower_dev, const double *upper_dev, double *inout_dev);
int mi_fvm_laplacian(mi_addr_t addr, const double *delta_coeffs_dev, const double *gamma_magsf_dev,
                     double *upper_out_dev, double *diag_out_dev);
int mi_fvm_div(mi_addr_t addr, const double *weights_dev, const double *face_flux_dev,
               double *lower_out_dev, double *upper_out_dev, double *diag_out_dev);
int mi_surface_integrate(mi_addr_t addr, const double *ssf_dev, const double *vol_dev_or_null, double *ivf_dev);
int mi_face_interpolate(mi_addr_t addr, const double *lambda_dev, const double *phi_dev, double *sf_dev);
/* ---- scheme front-end either side of the matrix ----
 * mi_fvm_ddt_euler: EulerDdtScheme fvmDdt (src/finiteVolume/finiteVolume/ddtSchemes/EulerDdtScheme/EulerDdtScheme.C):
 *   diag = rDeltaT*rho*V, source = rDeltaT*rho*psiOld*V (rho = 1 for the plain form).
 * mi_upwind_weights: pos(faceFlux) (limitedSchemes/upwind, limitedSurfaceInterpolationScheme.C:177-187).
 * mi_limited_linear_weights: limitedLinear(k) weights of a scalar field in one face pass -- r of
 *   limitedSchemes/LimitedScheme/NVDTVD.H, limiter of limitedSchemes/limitedLinear/limitedLinear.H:79-97, weights of
 *   limitedSurfaceInterpolationScheme.C:177-187; grad = cell gradient of phi (component arrays), c = cell centres;
 *   limiter_out may be NULL.  The result feeds mi_fvm_div / mi_face_interpolate.
 * mi_gauss_grad: fvc::grad with Gauss integration (finiteVolume/gradSchemes/gaussGrad/gaussGrad.C:27-90,143-250):
 *   g = (sum_own Sf*ssf - sum_nei Sf*ssf)/V over the internal faces, component arrays; boundary faces are added with
 *   mi_patch_add per component (vol = NULL here, then divide) exactly as the reference adds them per patch.
 * mi_vec_axpby: out = a*x + b*y (fvMatrix operator+=, -=, *= on coefficient arrays; out may alias x or y).        */
int mi_fvm_ddt_euler(mi_ctx_t ctx, int64_t n, double r_delta_t, double rho, const double *vol_dev,
                     const double *psi_old_dev, double *diag_out_dev, double *source_out_dev);
int mi_upwind_weights(mi_ctx_t ctx, int64_t n_faces, const double *face_flux_dev, double *weights_out_dev);
int mi_limited_linear_weights(mi_addr_t addr, double k, const double *cd_weights_dev, const double *face_flux_dev,
                              const double *phi_dev, const double *gradx_dev, const double *grady_dev,
                              const double *gradz_dev, const double *cx_dev, const double *cy_dev,
                              const double *cz_dev, double *weights_out_dev, double *limiter_out_dev_or_null);
/* ---- the TVD/NVD limited schemes and their V and bounded forms (finiteVolume/Make/files:253-273, limitedSchemes/<scheme>/<scheme>.C) ----
 * mi_limiter_parse: host only, no GPU.  Accepts exactly the names the reference registers -- limitedLinear vanLeer MUSCL Minmod SuperBee
 *   UMIST vanAlbada OSPRE QUICK limitedCubic Gamma SFCD, each with a "V" form (limitedLinearV ... SFCDV: NVDVTVDV.H), and the bounded
 *   forms of Limited.H / Limited01.H: limitedLimitedLinear k lo hi, limitedLinear01 k, limitedVanLeer lo hi, vanLeer01, limitedMUSCL lo hi,
 *   MUSCL01, limitedLimitedCubic k lo hi, limitedCubic01 k, limitedGamma k lo hi, Gamma01 k.  limitedLinear, limitedCubic and Gamma read
 *   k first.  Refused (MI_ERR_ARG): any other name, a missing or extra coefficient, k outside [0, 1] (limitedLinear.H:67-73,
 *   limitedCubic.H:67-73, Gamma.H:66-72), lower > upper (Limited.H:54-64), a bounded V form.
 * mi_limited_weights: LimitedSchemeCalcLimiterFunctor (LimitedScheme.C:32-57,88-136) + limitedSurfaceInterpolationSchemeWeightsFunctor
 *   (limitedSurfaceInterpolationScheme.C:155-161) on the internal faces in ONE face pass: d = C[N] - C[P], the limiter of lim->kind over
 *   NVDTVD.H (scalar: phi_dev[0], grad_dev[0..2]) or NVDVTVDV.H (vector_form: phi_dev[0..2], grad_dev[3*j + k] = d(phi_j)/dx_k), the
 *   LimitedLimiter bounds (Limited.H:105-118; a zero flux is in neither branch), then w = lim*cdw + (1 - lim)*pos(faceFlux).  Contraction:
 *   DESIGN 3.5b.  limiter_out may be NULL.  A vector field under a non-V scheme is limited on magSqr(U) (LimitFuncs.C:39-54): the caller
 *   forms that scalar and its gradient.  mi_limited_linear_weights stays the limitedLinear-only call.
 * mi_patch_limited_weights: the same on one COUPLED patch (LimitedScheme.C:145-195): phiP, gradcP through the patch's faceCells, phiN,
 *   gradcN the patchNeighbourField (mi_matrix_patch_neighbour_field per component), d = patch().delta() (patch_delta_dev, 3 component
 *   arrays), the patch's own CD weights and flux.  Non-coupled patches take limiter 1 (LimitedScheme.C:197-200): their weights ARE the
 *   patch CD weights, no call is needed.
 * Both refuse (MI_ERR_ARG, nothing launched): an invalid mi_limiter, missing arrays, unaligned face fields, outputs that alias an input. */
enum { MI_LIM_LIMITED_LINEAR, MI_LIM_VAN_LEER, MI_LIM_MUSCL, MI_LIM_MINMOD, MI_LIM_SUPERBEE, MI_LIM_UMIST,
       MI_LIM_VAN_ALBADA, MI_LIM_OSPRE, MI_LIM_QUICK, MI_LIM_LIMITED_CUBIC, MI_LIM_GAMMA, MI_LIM_SFCD };
typedef struct mi_limiter {
    int32_t kind;          /* MI_LIM_* */
    int32_t vector_form;   /* 0: NVDTVD over a scalar (1 phi, 3 grad arrays); 1: NVDVTVDV, the "...V" schemes (3 phi, 9 grad: grad[3*j+k] = d(phi_j)/dx_k) */
    int32_t bounded;       /* Limited.H: limitedX lo hi / X01; scalar form only */
    double k, lower, upper;
} mi_limiter;
int mi_limiter_parse(const char *scheme, mi_limiter *out);
int mi_limited_weights(mi_addr_t addr, const mi_limiter *lim, const double *cd_weights_dev, const double *face_flux_dev,
                       const double *const *phi_dev, const double *const *grad_dev, const double *const *c_dev,
                       double *weights_out_dev, double *limiter_out_dev_or_null);
int mi_patch_limited_weights(mi_patch_t patch, const mi_limiter *lim, const double *patch_cd_weights_dev, const double *patch_flux_dev,
                             const double *const *phi_dev, const double *const *nbr_phi_dev, const double *const *grad_dev,
                             const double *const *nbr_grad_dev, const double *const *patch_delta_dev,
                             double *weights_out_dev, double *limiter_out_dev_or_null);
/* ---- the filtered centred limiters of resolved (LES / DNS) runs: filteredLinear, filteredLinear2[V] k l, filteredLinear3[V] k ----
 * LimitedScheme limiters that remove staggering from a centred scheme (limitedSchemes/filteredLinear/filteredLinear.H:69-94 and .C:33-37,
 * filteredLinear2/filteredLinear2.H:80-141, filteredLinear2V.H:80-152 and filteredLinear2.C:34-44, filteredLinear3/filteredLinear3.H:72-107,
 * filteredLinear3V.H:72-112 and filteredLinear3.C:34-44).  Every one reads the gradient at BOTH cells of a face and none reads the flux: only
 * the weight blend does.  With d = C[N] - C[P] (the patch delta on a coupled patch), dc = d & gradc the dot product of every face pass here
 * (fma(dz, gz, fma(dx, gx, dy*gy)); V forms: dfV = phiN - phiP, df = dfV & dfV and dc = dfV & (d & gradc), component j of the inner
 * product d & grad(phi_j)), max / min the reference's ternaries ((a > b) ? a : b: max(-0.0, 0) = +0.0), SMALL = 1e-15, VSMALL = 1e-300,
 * and 2*x, 0.5*x exact, the limiters are -- no product-plus-sum in them to contract, evaluated left to right as parenthesised:
 *   filteredLinear        df = phiN - phiP:  max(min(2 - (0.5*min(|df - dcP|, |df - dcN|))/(max(|dcP|, |dcN|) + SMALL), 1), 0.8)
 *   filteredLinear2[V]    tdc = 2*dc, l_ = l + 1.0 (the constructor):  m = df > 0 ? min(max(df - tdcP, 0), max(df - tdcN, 0))
 *                         : min(max(tdcP - df, 0), max(tdcN - df, 0));  max(min(l_ - (k*m)/(max(|df|, max(|tdcP|, |tdcN|)) + SMALL), 1), 0)
 *                         (filteredLinear2V adds VSMALL where the scalar form adds SMALL)
 *   filteredLinear3[V]    dP = 2*dcP, dN = 2*dcN:  max(min(1 - ((k*(dN - df))*(dP - df))/max((dN + dP)*(dN + dP), SMALL), 1), 0)
 *                         (filteredLinear3V uses SMALL too)
 * then w = fma(lim, cdw, (1 - lim)*pos(faceFlux)) as mi_limited_weights.
 * mi_filtered_parse: host only, no GPU.  Accepts exactly the five registered names with 0, 2, 2, 1, 1 coefficients; l is kept as written in
 *   the case (the engine adds the constructor's 1.0).  Refused (MI_ERR_ARG, *out untouched): any other name (filteredLinearV, a name of
 *   mi_limiter_parse, ...), a missing or extra coefficient, a coefficient that is not a number, k or l outside [0, 1] as the constructors do.
 *   mi_limiter_parse keeps refusing these names: a filtered scheme is no mi_limiter.
 * mi_filtered_weights / mi_patch_filtered_weights: the face pass and the coupled-patch pass of mi_limited_weights / mi_patch_limited_weights
 *   (the same kernels, further kinds) with the same argument conventions -- scalar form 1 phi and 3 grad arrays, V form 3 and 9 with
 *   grad[3*j + k] = d(phi_j)/dx_k; limiter_out may be NULL -- and the same refusals, nothing launched: an invalid struct (kind, vector_form
 *   on filteredLinear, k or l out of range), missing arrays, unaligned face fields, an output that aliases an input.  Non-coupled patches
 *   take limiter 1: no call is needed. */
enum { MI_FLT_LINEAR, MI_FLT_LINEAR2, MI_FLT_LINEAR3 };
typedef struct mi_filtered_limiter {
    int32_t kind;          /* MI_FLT_* */
    int32_t vector_form;   /* 1: filteredLinear2V / filteredLinear3V (3 phi, 9 grad arrays); filteredLinear has none */
    double k, l;           /* l as written in the case; read by filteredLinear2[V] only, k by all but filteredLinear */
} mi_filtered_limiter;
int mi_filtered_parse(const char *scheme, mi_filtered_limiter *out);
int mi_filtered_weights(mi_addr_t addr, const mi_filtered_limiter *lim, const double *cd_weights_dev, const double *face_flux_dev,
                        const double *const *phi_dev, const double *const *grad_dev, const double *const *c_dev,
                        double *weights_out_dev, double *limiter_out_dev_or_null);
int mi_patch_filtered_weights(mi_patch_t patch, const mi_filtered_limiter *lim, const double *patch_cd_weights_dev, const double *patch_flux_dev,
                              const double *const *phi_dev, const double *const *nbr_phi_dev, const double *const *grad_dev,
                              const double *const *nbr_grad_dev, const double *const *patch_delta_dev,
                              double *weights_out_dev, double *limiter_out_dev_or_null);
int mi_gauss_grad(mi_addr_t addr, const double *sfx_dev, const double *sfy_dev, const double *sfz_dev,
                  const double *ssf_dev, const double *vol_dev_or_null, double *gx_dev, double *gy_dev, double *gz_dev);
/* ---- the limited gradient schemes (finiteVolume/gradSchemes/limitedGradSchemes: cellLimitedGrad, cellMDLimitedGrad, faceLimitedGrad, faceMDLimitedGrad) ----
 * mi_grad_limiter_parse: host only, no GPU.  Accepts exactly `cellLimited|cellMDLimited|faceLimited|faceMDLimited Gauss linear <k>` (the
 *   constructors read the base scheme through gradScheme::New, then readScalar: cellLimitedGrad.H:88-107 and its siblings).  Refused
 *   (MI_ERR_ARG): any other name, a base other than Gauss, an interpolation other than linear, a limited scheme over a limited scheme, a
 *   missing or extra token, k outside [0, 1].  identity = k < SMALL (1e-15): the basic scheme's gradient is returned unchanged.
 * mi_grad_boundary_create: the boundary as the limiters see it, built once per mesh on the host: n_patches patches in the reference's
 *   order, patch p with patch_sizes[p] faces whose cells are face_cells_host[p], of kind patch_kinds[p] (MI_GRAD_PATCH_*: coupled,
 *   fixesValue() or any other; an empty patch has zero faces).  Boundary face fields are the patch-ordered concatenation of every patch's
 *   faces (nb = sum of patch_sizes).
 * mi_limited_grad: limits the internal field of a Gauss linear gradient in place (grad_inout_dev[3*j + k] = d(vf_j)/dx_k, from
 *   mi_gauss_grad + the boundary faces + the division by V), for n_comp = 1 (scalar) or 3 (vector) components, in ONE row pass:
 *   cellLimited (cellLimitedGrads.C:47-199 scalar, :201-364 vector; limitFace cellLimitedGrad.H:136-171), cellMDLimited
 *   (cellMDLimitedGrads.C; cellMDLimitedGrad.H:136-180), faceLimited (faceLimitedGrads.C:47-177 scalar, :183-340 vector; faceLimitedGrad.H:140-156,
 *   including the vector form's unexpanded bounds on the neighbour side of an internal face, :241-254) and faceMDLimited (faceMDLimitedGrads.C).
 *   c_dev: cell centres [x, y, z]; cf_dev: internal face centres; bvalue_dev[j]: per boundary face the patchNeighbourField (coupled
 *   patches, e.g. mi_matrix_patch_neighbour_field) or the boundary value (the others); bcf_dev: boundary face centres.  The cell kinds
 *   read every patch, the face kinds the coupled and fixesValue patches only.  boundary NULL: no boundary faces.  limiter_out: n_comp
 *   cell arrays for cellLimited, 1 for faceLimited, NULL for the MD kinds (or NULL).  Each cell's faces are visited in the reference's
 *   order and every expression is rounded as the reference's host loops round it.  With lim->identity nothing is written
 *   and nothing launched.  Refused (MI_ERR_ARG, nothing launched): an invalid mi_grad_limiter, n_comp not 1 or 3, a boundary built for
 *   another addressing, NULL boundary arrays while the boundary has faces, limiter_out for an MD kind, missing arrays, an output that
 *   aliases an input or another output.  The gradient's boundary values stay the caller's (as for mi_gauss_grad). */
enum { MI_GRAD_CELL_LIMITED, MI_GRAD_CELL_MD_LIMITED, MI_GRAD_FACE_LIMITED, MI_GRAD_FACE_MD_LIMITED };
enum { MI_GRAD_PATCH_OTHER, MI_GRAD_PATCH_COUPLED, MI_GRAD_PATCH_FIXES_VALUE };
typedef struct mi_grad_limiter {
    int32_t kind;          /* MI_GRAD_* */
    int32_t identity;      /* k < SMALL */
    double k;
} mi_grad_limiter;
typedef struct mi_grad_boundary_s *mi_grad_boundary_t;
int mi_grad_limiter_parse(const char *scheme, mi_grad_limiter *out);
int mi_grad_boundary_create(mi_addr_t addr, int32_t n_patches, const int32_t *patch_sizes, const int32_t *const *face_cells_host,
                            const int32_t *patch_kinds, mi_grad_boundary_t *out);
int mi_grad_boundary_destroy(mi_grad_boundary_t boundary);
int mi_limited_grad(mi_addr_t addr, const mi_grad_limiter *lim, mi_grad_boundary_t boundary_or_null, int32_t n_comp,
                    const double *const *vf_dev, const double *const *c_dev, const double *const *cf_dev, const double *const *bvalue_dev,
                    const double *const *bcf_dev, double *const *grad_inout_dev, double *const *limiter_out_dev_or_null);
/* ---- the leastSquares gradient scheme (finiteVolume/gradSchemes/leastSquaresGrad: leastSquaresVectors.C, leastSquaresGrad.C) ----
 * The reference's device code for this scheme cannot be the definition (leastSquaresGrad.C:120-136 writes through a permutation iterator
 * whose indices repeat and reads ownLs where the loop it replaces reads neiLs; leastSquaresVectors.C:85-98 does not compile; SURVEY
 * Appendix B).  The definition is what the two files keep of the upstream algorithm; it is restated in tests/test_least_squares_grad.py,
 * not pinned by a compiled reference.
 * mi_grad_scheme_parse: host only, no GPU.  The gradSchemes entry: accepts exactly `Gauss linear`, `leastSquares` and
 *   `cellLimited|cellMDLimited|faceLimited|faceMDLimited <Gauss linear|leastSquares> <k>` (gradScheme::New, gradScheme.C:34-77; the limited
 *   constructors cellLimitedGrad.H:88-107 and siblings).  A limited entry fills `limiter` exactly as mi_grad_limiter_parse does (same k range,
 *   identity, whitespace rules); an unlimited one leaves it zero.  Refused (MI_ERR_ARG): any other base (fourth, ...), another
 *   interpolation, a limited scheme over a limited one, a trailing token after leastSquares, a missing or extra coefficient, an empty string.
 *   mi_grad_limiter_parse keeps its narrower grammar.
 * mi_ls_vectors_create: the least-squares vectors of one mesh, built once on the device (leastSquaresVectors.C:123-225, the host loops):
 *   dd[c] summed per cell in the loops' order -- internal faces in face order (neighbour side w*wdd, owner side (1 - w)*wdd,
 *   wdd = (magSf/magSqr(d))*sqr(d), d = C[nei] - C[own]), then the patches in patch order (coupled: ((1 - pw)*pMagSf/magSqr(d))*sqr(d),
 *   the others (pMagSf/magSqr(d))*sqr(d), d = p.delta() as the caller supplies it) -- then inv(dd) in the host Field<symmTensor> form
 *   (symmTensorField.C:50-105): CALLER CELL 0 ALONE decides removeCmpts (magSqr(dd[0].cc)/magSqr(dd[0]) < SMALL), a removed component gets
 *   +1 before and -1 after the inversion in every cell (one 48-byte read-back; this is what makes a one-cell-thick mesh with empty patches
 *   work), the inversion itself SymmTensorI.H:344-399; then pVectors = (1 - w)*magSfByMagSqrd*(invDd[own] & d), nVectors =
 *   -w*magSfByMagSqrd*(invDd[nei] & d) and the boundary pVectors (:190-225).  Every expression is rounded operation by operation, left to
 *   right as written.  c_dev: cell centres [x, y, z]; weights_dev / mag_sf_dev: internal faces; b_*: boundary face fields,
 *   the patch-ordered concatenation of `boundary` (MI_GRAD_PATCH_COUPLED takes the coupled branch, FIXES_VALUE and OTHER the other one;
 *   b_weights is read on coupled faces only and may be NULL without them).  boundary NULL: no boundary faces; otherwise it must outlive the
 *   handle.  A mesh or a cell without faces is legal: such a cell's inverse is not finite and is read by nobody.
 * mi_ls_vectors_fields: copies the vectors out (LeastSquaresP / LeastSquaresN and the boundary field of LeastSquaresP), three arrays each,
 *   the caller's face order; bp_out may be NULL when the boundary has no faces.
 * mi_ls_grad: the gradient's internal field in ONE row pass (grad_out_dev[3*j + k] = d(vf_j)/dx_k, n_comp = 1 or 3): the loop of
 *   leastSquaresGrad.C:109-118 then the patches (:139-189) with the arithmetic of leastSquaresCalcGradFunctor (:39-53) contracted as every
 *   device functor is (inferred, not pinned): delta rounded once, then grad[3*j + k] = fma(+-ls_k, delta_j, grad[3*j + k]).
 *   Per cell: the neighbour-side faces ascending (nVectors, delta = vf[c] - vf[own(f)], fma(-ls_k, ...)), its own faces ascending
 *   (pVectors, delta = vf[nei(f)] - vf[c]), its boundary faces by patch and face (fma(bLs_k, bvalue - vf[c], g_k)); no division by V; a
 *   cell without faces gets +0.  bvalue_dev[j]: per boundary face the patchNeighbourField (coupled) or the boundary value (the others), as
 *   for mi_limited_grad.  The gradient's boundary values stay the caller's (mi_patch_gauss_grad_correct, which leastSquaresGrad.C:193 calls too).
 *   A limited leastSquares gradient is mi_ls_grad followed by mi_limited_grad (cellLimitedGrad::calcGrad takes any basicGradScheme_).
 * Refused (MI_ERR_ARG, nothing launched): n_comp not 1 or 3, a missing array, a boundary built for another addressing, NULL boundary
 *   arrays while the boundary has faces, an output that aliases an input or another output. */
enum { MI_GRAD_BASE_GAUSS_LINEAR, MI_GRAD_BASE_LEAST_SQUARES };
typedef struct mi_grad_scheme {
    int32_t base;          /* MI_GRAD_BASE_* */
    int32_t limited;       /* 1: `limiter` holds the limited scheme wrapped around the base */
    mi_grad_limiter limiter;
} mi_grad_scheme;
typedef struct mi_ls_vectors_s *mi_ls_vectors_t;
int mi_grad_scheme_parse(const char *scheme, mi_grad_scheme *out);
int mi_ls_vectors_create(mi_addr_t addr, mi_grad_boundary_t boundary_or_null, const double *const *c_dev, const double *weights_dev,
                         const double *mag_sf_dev, const double *b_weights_dev, const double *b_mag_sf_dev, const double *const *b_delta_dev,
                         mi_ls_vectors_t *out);
int mi_ls_vectors_destroy(mi_ls_vectors_t lsv);
int mi_ls_vectors_fields(mi_ls_vectors_t lsv, double *const *p_out_dev, double *const *n_out_dev, double *const *bp_out_dev_or_null);
int mi_ls_grad(mi_ls_vectors_t lsv, int32_t n_comp, const double *const *vf_dev, const double *const *bvalue_dev_or_null,
               double *const *grad_out_dev);
/* ---- fvc::surfaceSum and fvc::reconstruct: a face flux back to a cell vector (finiteVolume/fvc/fvcReconstruct.C:45-84) ----
 * The pEqn.H / UEqn.H line of the buoyant and multiphase solvers, U = HbyA + rAU*fvc::reconstruct((phig - p_rghEqn.flux())/rhorAUf).  The
 * reference evaluates inv(surfaceSum(SfHat*mesh.Sf())) & surfaceSum(SfHat*ssf), SfHat = Sf/magSf, and re-forms and re-inverts the geometric
 * tensor on every call; on a static mesh it is a constant, built here once per mesh.  Restated in tests/reconstruct_support.py, not pinned by
 * a compiled reference.
 * Order (fvcSurfaceIntegrate.C:262-360 with surfaceIntegrateFunctor<Type, false>, :40-132): a cell starts from +0.0 and meets its own faces
 *   ascending, its neighbour-side faces in losort order, then its boundary faces by patch and by face within the patch
 *   (surfaceIntegratePatchFunctor's running add).  Every term is ADDED on both sides, unlike surfaceIntegrate.  Coupled patches are added
 *   like any other and no neighbour value is read: an attached (decomposed) matrix needs no communication.
 * mi_surface_sum: out[c] = the sum of ssf[f] (MI_SURFACE_SUM) or of |ssf[f]| (MI_SURFACE_SUM_MAG: the fvc::surfaceSum(mag(phi)) of
 *   CourantNo.H) over the internal faces of c in that order -- the row pass of mi_row_face_op kind 0 / kind 2 with lower NULL started from
 *   +0.0 (no new kernel).  Boundary faces are then added per patch with mi_patch_add (fn 0 / fn 2), as for mi_gauss_grad.
 * mi_reconstruct_create: SfHat_k = Sf_k/magSf (one division per component, internal and boundary faces alike), the geometric tensor
 *   T_ab[c] = sum_f SfHat_a[f]*Sf_b[f] -- NINE components (T_xy and T_yx may differ in the last bit), each product rounded, then added in
 *   the order above -- and its inverse in the device Field<tensor> form (tensorField.C:226-305): CALLER CELL 0 ALONE decides removeCmpts
 *   (scale = magSqr(T[0]), the nine squares summed left to right xx xy xz yx yy yz zx zy zz; x is removed when T[0].xx/scale < SMALL = 1e-15,
 *   likewise y and z; a cell 0 without faces gives 0/0, the comparison is false and nothing is removed; one 72-byte read-back); a removed
 *   component adds the whole tensor (1,0,0, 0,0,0, 0,0,0) ... to every cell before the inversion and subtracts it after (the zeros are added
 *   too: a -0.0 component becomes +0.0; this is what makes a one-cell-thick mesh with empty patches work); det as TensorI.H:552-560, left to
 *   right, the inverse the nine cofactor expressions of :588-604, each divided by det.  Every operation is rounded on its own (DESIGN 3.5c /
 *   3.5i); that the reference's device functor is not contracted is an ASSUMPTION.  sf_dev [x, y, z] / mag_sf_dev: internal
 *   faces; b_*: boundary face fields, the patch-ordered concatenation of `boundary` (mi_grad_boundary_create; the patch kinds are not read).
 *   boundary NULL: no boundary faces; otherwise it must outlive the handle.  The caller's geometry arrays are not kept.  The handle owns
 *   SfHat (internal and boundary) and the nine inverse arrays: 24F + 72N + 24nb bytes, about 1.45 GB at 216^3.  After mesh motion: destroy
 *   and create.  Works under the caller's numbering and under mi_addr_create_ordered, as mi_ls_grad does.
 * mi_reconstruct_fields: copies the inverse out, nine cell arrays xx xy xz yx yy yz zx zy zz, and removeCmpts as three 0 / 1 host values
 *   (removed_out_host may be NULL).
 * mi_fvc_reconstruct: n_rhs = 1..4 fluxes in ONE row pass (out_dev[3*r + k] = component k of reconstruct(ssf_r)): s_k[c] = sum_f
 *   SfHat_k[f]*ssf[f], the product rounded, then added, in the order above; out_a = row a of T^-1 dotted with s as the engine's dot product
 *   (the same standing assumption): fma(R_az, s_z, fma(R_ax, s_x, R_ay*s_y)).  No division by V.  The pass reads 24 bytes
 *   of geometry per face and performs no division.  b_ssf_dev[r]: the boundary fluxes, patch-ordered; may be NULL without boundary faces.
 *   A cell without faces has T = 0 and det = 0: its inverse and output are not finite, which is legal.  The result's boundary values
 *   (zeroGradient: mi_patch_internal_field; coupled patches through the neighbour-field entries) stay the caller's, as for every gradient.
 * Refused (MI_ERR_ARG, nothing launched, nothing written): n_rhs outside 1..4, a mode other than the two, a missing array or one not
 *   aligned for a double, a boundary built for another addressing, NULL boundary arrays while the boundary has faces, an output that aliases
 *   an input or another output.  Zero cells: MI_OK, nothing written.  Zero internal faces is legal (the face arrays may be NULL).
 * Out of scope: reconstruct of a surfaceVectorField (tensor result), fvc::reconstructMag, fvc::curl, a Courant-number entry (its max
 *   is mi_min_max below), moving meshes. */
typedef struct mi_reconstruct_s *mi_reconstruct_t;
enum { MI_SURFACE_SUM, MI_SURFACE_SUM_MAG };
int mi_surface_sum(mi_addr_t addr, int32_t mode, const double *ssf_dev, double *out_dev);
int mi_reconstruct_create(mi_addr_t addr, mi_grad_boundary_t boundary_or_null, const double *const *sf_dev, const double *mag_sf_dev,
                          const double *const *b_sf_dev, const double *b_mag_sf_dev, mi_reconstruct_t *out);
int mi_reconstruct_destroy(mi_reconstruct_t rc);
int mi_reconstruct_fields(mi_reconstruct_t rc, double *const *inv_out_dev, int32_t *removed_out_host);
int mi_fvc_reconstruct(mi_reconstruct_t rc, int32_t n_rhs, const double *const *ssf_dev, const double *const *b_ssf_dev_or_null,
                       double *const *out_dev);
int mi_vec_axpby(mi_ctx_t ctx, int64_t n, double a, const double *x_dev, double b, const double *y_dev, double *out_dev);
/* ---- explicit MULES: limiter, limit and explicitSolve (finiteVolume/fvMatrices/solvers/MULES/MULESTemplates.C:36-813, MULESFunctors.H;
 *      DESIGN 3.5l) ----
 * What every VOF solver of the reference (interFoam and its family) advances its phase fraction with.  The reference spends more than 60
 * launches on one limit + explicitSolve; here it is one row pass to open, one row pass and one face pass per limiter iteration, one face
 * pass to apply and one row pass to solve.  Restated in tests/mules_support.py, not pinned by a compiled reference.
 * Order: a cell meets its own faces ascending, its neighbour-side faces in losort order, then its boundary faces by patch and by face, as
 *   in mi_fvc_reconstruct.  Every operation is rounded on its own; max / min are (a > b) ? a : b and (a < b) ? a : b.
 * mi_mules_create: the handle of one mesh.  boundary NULL: no boundary faces; otherwise it must outlive the handle.  Its
 *   MI_GRAD_PATCH_COUPLED patches take the coupled rules (psiPf = patchNeighbourField; lambda from the face cell by the sign of phiCorr),
 *   FIXES_VALUE and OTHER the rule of every other patch (limited only where phiBD + phiCorr > SMALL*SMALL).
 *   patch_is_wedge_host_or_null[p] != 0 marks patch p a wedge patch (lambda = 0 after every iteration) whatever its kind.  The handle owns
 *   six cell arrays -- the transformed bounds psiMaxn and psiMinn, sumPhip, mSumPhim, lambdap, lambdam -- and one byte and one label per
 *   boundary face, so no call allocates.  mi_mules_work copies the six arrays out in that order.
 * mi_mules_fields: r_delta_t, or r_delta_t_dev per cell (explicitLTSSolve) when not NULL; rho_dev and rho_old_dev, both or neither
 *   (neither: geometricOneField); sp_dev / su_dev or NULL (zeroField); an absent term's operation is NOT performed (one*x = x,
 *   x - zero = x, zero - x = -x), so a -0.0 survives where 0.0 - x would lose it.  vol_dev, psi_dev, psi_old_dev: cell arrays.
 *   b_psi_dev: per boundary face the patchNeighbourField (coupled patches) or the patch value, patch-ordered as mi_limited_grad's bvalue.
 * mi_mules_flux: the face arrays, each with its patch-ordered boundary twin b_*.  Which of them a call reads or writes is listed below;
 *   the others are not looked at.
 * mi_mules_begin: form MI_MULES_LIMITER takes phi_bd / phi_corr as given and leaves lambda as given (MULES::limiter's arguments);
 *   MI_MULES_LIMIT reads phi and phi_psi and WRITES phi_bd = phi*(w*(psiP - psiN) + psiN) with w = pos(phi) (coupled patch faces:
 *   phi*(w*psiInternal + (1 - w)*psiNeighbour); other patch faces: phi*psiPf), phi_corr = phi_psi - phi_bd and lambda = 1.  Either way it
 *   then fills psiMaxn / psiMinn (from psi_min / psi_max over the NEIGHBOUR cells and the boundary psiPf -- the cell's own value is not
 *   among them --, clamped by psi_max / psi_min, then the static-mesh expressions of :538-554), sumPhip and mSumPhim (from VSMALL;
 *   `phiCorr > 0.0` picks the branch).
 * mi_mules_iterate: n limiter iterations, lambda in place: sumlPhip / mSumlPhim over lambda*phi_corr, lambdam = max(min((sumlPhip +
 *   psiMaxn)/(mSumPhim - SMALL), 1), 0), lambdap = max(min((mSumlPhim + psiMinn)/(sumPhip + SMALL), 1), 0), then per face min(lambda, ...)
 *   by the sign of phi_corr.  The syncFaceList(minOp) that ends an iteration needs the other side of a coupled face and is the CALLER's:
 *   on a boundary with coupled patches iterate one at a time and take the minimum of the two sides (mi_vec_min) after each.
 * mi_mules_apply: out = phi_bd + lambda*phi_corr, or lambda*phi_corr with return_corr, the product rounded first.  out may be the array
 *   that was phi_psi (the reference overwrites phiPsi).
 * mi_mules_limiter = begin(MI_MULES_LIMITER) + iterate(n_limiter_iter); mi_mules_limit = begin(MI_MULES_LIMIT) + iterate + apply; 3 is
 *   what MULES::explicitSolve passes.  mi_mules_explicit_solve: psi_out = (rho_old*psi_old*rDeltaT + Su - surfaceIntegrate(phi_psi))
 *   /(rho*rDeltaT - Sp), surfaceIntegrate being own +, neighbour side -, boundary +, then /V.  It needs no begin and reads no psi_dev, which may be NULL or psi_out itself (the reference overwrites psi).
 * mi_vec_min: out = (x < y) ? x : y element by element (out may alias x or y): minOp over the two patch slices of a one-rank cyclic pair.
 * Refused (MI_ERR_ARG, nothing launched, nothing written): a handle or boundary of another addressing, missing arrays, NULL boundary
 *   arrays while the boundary has faces, an array not aligned for a double, an output that aliases an input or another output, rho
 *   without rho_old (or the reverse), n < 0, iterate or apply before begin, an unknown form, and -- on a boundary with coupled patches --
 *   iterate with n > 1, mi_mules_limiter and mi_mules_limit.  Zero cells: MI_OK.  Zero internal faces is legal (the face arrays may be NULL).
 * Out of scope: IMULES, limitSum, moving meshes (Vsc0), the minOp sync across ranks.  CMULES and interfaceCompression: below. */
typedef struct mi_mules_s *mi_mules_t;
enum { MI_MULES_LIMITER, MI_MULES_LIMIT };
typedef struct mi_mules_fields {
    double r_delta_t;
    const double *r_delta_t_dev;              /* per cell, or NULL: r_delta_t */
    const double *rho_dev, *rho_old_dev;      /* both or neither */
    const double *sp_dev, *su_dev;            /* each or NULL */
    const double *vol_dev, *psi_dev, *psi_old_dev;
    const double *b_psi_dev;
    double psi_max, psi_min;
} mi_mules_fields;
typedef struct mi_mules_flux {
    const double *phi_dev, *b_phi_dev;          /* begin(MI_MULES_LIMIT): read */
    const double *phi_psi_dev, *b_phi_psi_dev;  /* begin(MI_MULES_LIMIT): read */
    double *phi_bd_dev, *b_phi_bd_dev;          /* begin(MI_MULES_LIMIT): written; otherwise read */
    double *phi_corr_dev, *b_phi_corr_dev;      /* likewise */
    double *lambda_dev, *b_lambda_dev;          /* begin(MI_MULES_LIMIT): written; iterate: read and written; otherwise read */
    double *out_dev, *b_out_dev;                /* apply: written */
} mi_mules_flux;
int mi_mules_create(mi_addr_t addr, mi_grad_boundary_t boundary_or_null, const int32_t *patch_is_wedge_host_or_null, mi_mules_t *out);
int mi_mules_destroy(mi_mules_t mules);
int mi_mules_work(mi_mules_t mules, double *const *out_dev);
int mi_mules_begin(mi_mules_t mules, int32_t form, const mi_mules_fields *fields, const mi_mules_flux *flux);
int mi_mules_iterate(mi_mules_t mules, int32_t n, const mi_mules_fields *fields, const mi_mules_flux *flux);
int mi_mules_apply(mi_mules_t mules, int32_t return_corr, const mi_mules_fields *fields, const mi_mules_flux *flux);
int mi_mules_limiter(mi_mules_t mules, int32_t n_limiter_iter, const mi_mules_fields *fields, const mi_mules_flux *flux);
int mi_mules_limit(mi_mules_t mules, int32_t n_limiter_iter, int32_t return_corr, const mi_mules_fields *fields, const mi_mules_flux *flux);
int mi_mules_explicit_solve(mi_mules_t mules, const mi_mules_fields *fields, const double *phi_psi_dev, const double *b_phi_psi_dev,
                            double *psi_out_dev);
int mi_vec_min(mi_ctx_t ctx, int64_t n, const double *x_dev, const double *y_dev, double *out_dev);
/* ---- semi-implicit MULES: limiterCorr, limitCorr and correct (CMULESTemplates.C:35-758, MULESFunctors.H) ----
 * What interFoam's alphaEqn.H runs with `MULESCorr yes`: MULES::correct(alpha1, phiAlphaUn, phiAlphaCorr, 1, 0) is mi_mules_limit_corr then
 * mi_mules_correct.  The handle, the fields, the flux arrays, the order of a cell's faces and the rounding rules are explicit MULES'; what
 * differs from it:
 * mi_mules_begin_corr: reads phi_corr, b_phi_corr, psi, b_psi, vol, rho, sp, su and rDeltaT; psi_old_dev, rho_old_dev, phi_bd and phi_psi
 *   are not looked at and may be NULL (rho without rho_old is legal here).  psiMaxn / psiMinn start from psi_min / psi_max and run over the
 *   NEIGHBOUR cells' psi and the boundary psiPf (the cell's own value is not among them); sumPhip / mSumPhim from VSMALL, `phiCorr > 0.0`
 *   picks the branch; there is no phiBD.  Clamp: psiMaxn = min(psiMaxn + e, psi_max), psiMinn = max(psiMinn - e, psi_min) with
 *   e = extrema_coeff*(psi_max - psi_min) formed once on the host; the addition is performed even when e is 0.0 (-0.0 + 0.0 = +0.0).  Then
 *   psiMaxn = V*((rho*rDeltaT - Sp)*psiMaxn - Su - rho*psi*rDeltaT), psiMinn = V*(Su - (rho*rDeltaT - Sp)*psiMinn + rho*psi*rDeltaT), one
 *   rounding per written operator left to right, the old-value term (rho*psi)*rDeltaT of the CURRENT psi and rho.  Form
 *   MI_MULES_CORR_LIMIT also writes lambda = 1; MI_MULES_CORR_LIMITER leaves lambda as given.
 * The handle remembers which begin opened it.  After mi_mules_begin_corr, mi_mules_iterate limits a face of a patch that is neither
 *   coupled nor wedge where the BOUNDARY VALUE OF phi (b_phi_dev) is > SMALL*SMALL (patchLambdaPfCMULESFunctor), not phiBD + phiCorr; it
 *   reads phi_corr, b_phi_corr and b_phi and never phi_dev or phi_bd.  mi_mules_apply then takes return_corr = 1 only (there is no phiBD)
 *   and accepts out_dev == phi_corr_dev and b_out_dev == b_phi_corr_dev (limitCorr's phiCorr *= lambda).  mi_mules_work is unchanged.
 * mi_mules_limiter_corr = begin_corr(MI_MULES_CORR_LIMITER) + iterate(n); mi_mules_limit_corr = begin_corr(MI_MULES_CORR_LIMIT) +
 *   iterate(n) + the product into phi_corr / b_phi_corr in place (out_dev / b_out_dev are not looked at).
 * mi_mules_correct: psi = (rho*psi*rDeltaT + Su - surfaceIntegrate(phi_corr))/(rho*rDeltaT - Sp) in place in psi_inout_dev; needs no begin;
 *   the fields' psi_dev, psi_old_dev, rho_old_dev and b_psi_dev are not looked at (each may be NULL).  psi_inout is the one permitted alias.
 * Refused as explicit MULES refuses, and: extrema_coeff negative or not finite, an unknown form, b_phi_dev NULL while the boundary has a
 *   face on a patch that is neither coupled nor wedge, return_corr = 0 after begin_corr.  Coupled patches: iterate(n > 1) and the two
 *   conveniences are refused, the minOp sync is the caller's.  No call allocates; no atomics; the same bits on every run. */
enum { MI_MULES_CORR_LIMITER, MI_MULES_CORR_LIMIT };
int mi_mules_begin_corr(mi_mules_t mules, int32_t form, double extrema_coeff, const mi_mules_fields *fields, const mi_mules_flux *flux);
int mi_mules_limiter_corr(mi_mules_t mules, int32_t n_limiter_iter, double extrema_coeff, const mi_mules_fields *fields, const mi_mules_flux *flux);
int mi_mules_limit_corr(mi_mules_t mules, int32_t n_limiter_iter, double extrema_coeff, const mi_mules_fields *fields, const mi_mules_flux *flux);
int mi_mules_correct(mi_mules_t mules, const mi_mules_fields *fields, const double *phi_corr_dev, const double *b_phi_corr_dev, double *psi_inout_dev);
/* ---- the interfaceCompression scheme and alphaEqn.H's compression flux (interfaceCompression.H:58-77, PhiScheme.C:52-197) ----
 * mi_interface_compression_parse: MI_OK for exactly "interfaceCompression" (PhiScheme takes no coefficient).
 * mi_interface_compression_weights: limiter = min(max(1 - max(sqr(1 - 4*aP*(1 - aP)), sqr(1 - 4*aN*(1 - aN))), 0), 1) from the two cell
 *   values alone, weights = limiter*cdw + (1 - limiter)*pos(faceFlux), the blend of mi_limited_weights; one face pass, no gradient and no
 *   centres.  Rounding (the device-functor rule of mi_limited_weights): 1 - (4*a)*(1 - a) is fma(-(4*a), 1 - a, 1), sqr a plain product,
 *   max / min the ternaries, the weights fma(limiter, cdw, (1 - limiter)*pos).  The flux is the volumetric one (the rho-weighted branch of
 *   PhiScheme.C:87-94 is the caller's).  Non-coupled patches take limiter 1: no call.  The patch form is for a COUPLED patch: alpha_dev the
 *   cell field (patchInternalField through the patch's faceCells), nbr_alpha_dev the patchNeighbourField.
 * mi_alpha_compression_flux: out = fvc::flux(-fvc::flux(-phir, alpha2, interfaceCompression), alpha1, interfaceCompression) with
 *   alpha2 = 1.0 - alpha1 per cell, in one face pass, with the bits of the unfused sequence: n = -phir; w2 = weights(cdw, n, alpha2);
 *   g = n*interpolate(w2, alpha2); m = -g; w1 = weights(cdw, m, alpha1); out = m*interpolate(w1, alpha1); interpolate the rule of
 *   mi_face_interpolate, on a coupled patch w*P + (1 - w)*N with every operator rounded.
 * Refused: missing arrays, an output that aliases an input or the other output, face arrays not aligned to 16 bytes (patch arrays and
 *   cell arrays: 8). */
int mi_interface_compression_parse(const char *scheme);
int mi_interface_compression_weights(mi_addr_t addr, const double *cd_weights_dev, const double *face_flux_dev, const double *alpha_dev,
                                     double *weights_out_dev, double *limiter_out_dev_or_null);
int mi_patch_interface_compression_weights(mi_patch_t patch, const double *patch_cd_weights_dev, const double *patch_flux_dev,
                                           const double *alpha_dev, const double *nbr_alpha_dev,
                                           double *weights_out_dev, double *limiter_out_dev_or_null);
int mi_alpha_compression_flux(mi_addr_t addr, const double *cd_weights_dev, const double *phir_dev, const double *alpha1_dev, double *out_dev);
int mi_patch_alpha_compression_flux(mi_patch_t patch, const double *patch_cd_weights_dev, const double *patch_phir_dev,
                                    const double *alpha1_dev, const double *nbr_alpha1_dev, double *out_dev);
/* ---- interFoam's interfaceProperties: nHatf, curvature and surface tension force (transportModels/interfaceProperties/
 *      interfaceProperties.C:58-159, :220-231) ----
 * What calculateK() and surfaceTensionForce() run as about twenty field passes with vector temporaries is two face passes and one row pass
 * here.  Every operator is rounded on its own except the fma written below; division and square root are the correctly rounded IEEE ones.
 * mi_interface_nhatf (internal faces; :127, :134, :143): with P = lower[f], N = upper[f], per component k
 *     g_k = fma(lambda, gP_k - gN_k, gN_k)                     (the rule of mi_face_interpolate)
 *     m = sqrt(fma(g_z, g_z, fma(g_x, g_x, g_y*g_y)))          (mag of a vector, the contraction of 3.5a: an assumption, see DESIGN)
 *     d = m + delta_n;  n_k = g_k/d                            (three divisions, no reciprocal)
 *     nHatf = fma(n_z, Sf_z, fma(n_x, Sf_x, n_y*Sf_y))
 *   grad_dev: the three cell arrays of a gradient entry; sf_dev: three face arrays; nhatfv_out_dev_or_null: three face arrays for n, or NULL.
 *   A zero gradient gives exactly 0/(0 + delta_n) = 0.  delta_n is the caller's (1e-8/cbrt(average(V)): a device reduction's order could
 *   not be the reference's).
 * mi_patch_interface_nhatf: one patch, three forms by what mi_patch_nhatf holds.
 *   patch_weights_dev given (a COUPLED patch): g_k = w*gP_k + (1 - w)*gNbr_k, every operator rounded; grad_dev the cell gradient (read
 *     through the patch's faceCells), nbr_grad_dev its patchNeighbourField.
 *   patch_weights_dev NULL: grad_dev holds the BOUNDARY VALUE of gradAlpha per patch face (mi_patch_gauss_grad_correct); no cell is read.
 *   theta_deg_dev given (a contact-angle patch; patch_weights_dev NULL only; patch_magsf_dev required): after n_k = g_k/d,
 *     correctContactAngle :83-111: theta = (pi/180.0)*theta_deg; nf_k = Sf_k/magSf; a12 = n & nf (the fma chain); b1 = cos(theta);
 *     b2 = cos(acos(a12) - theta); det = 1.0 - a12*a12; a = (b1 - a12*b2)/det; b = (b2 - a12*b1)/det; n_k = a*nf_k + b*n_k (two products
 *     and a sum, no fma); n_k /= (mag(n) + delta_n); gradient_out = (nf & n)*mag(g) when given.  |a12| >= 1 has no special case: NaN comes
 *     out as it does in the reference.  b1_out_dev / b2_out_dev (both or neither): the device's own cos / acos results, for tests.  The
 *     angle models' theta(U, nHat) and acap.evaluate() are the caller's.
 *   Then nHatf = n & Sf with the patch's Sf; nhatfv_out_dev all three or all NULL.
 * mi_interface_create / mi_interface_destroy: the handle of the curvature's row pass on one mesh, from a mi_grad_boundary_t (NULL: no
 *   boundary faces), which must outlive it.  mi_interface_curvature (:146): K = -fvc::div(nHatf) in one launch: per cell the sum over its
 *   own faces ascending (+), its neighbour-side faces in losort order (-), its boundary faces patch by patch (+, b_nhatf_dev patch-ordered
 *   as b_phi_psi_dev of mi_mules_explicit_solve), then /V, then a true sign flip: a cell without flux gives -0.0.  No atomics.
 * mi_surface_tension_force (:223): sP = sigma*K[P], sN = sigma*K[N] (sigmaK() is a cell product before the interpolate);
 *   i = fma(lambda, sP - sN, sN); sn = deltaCoeffs*(alpha[N] - alpha[P]), + sngrad_corr[f] when given (the explicit part of a corrected /
 *   limited snGrad: mi_sngrad_*correction_flux with a gammaMagSf of ones); out = i*sn.  mi_patch_surface_tension_force (a COUPLED patch):
 *   i = w*sP + (1 - w)*(sigma*nbrK), sn = pDeltaCoeffs*(nbrAlpha - alpha[faceCells]) [+ corr], the product.
 * mi_near_interface (:230): out = pos(alpha - 0.01)*pos(0.99 - alpha), pos(x) = (x >= 0) ? 1 : 0; out may be alpha.
 * Refused (MI_ERR_ARG, nothing launched, nothing written): delta_n not finite or <= 0; missing arrays; an output that aliases an input
 *   or another output; internal-face arrays not 16-byte aligned, cell and patch arrays not 8-byte aligned; theta_deg with patch_weights;
 *   the contact-angle form without patch_magsf; gradient_out / b1_out / b2_out without theta_deg; a handle of another addressing.
 *   Zero faces: MI_OK. */
typedef struct mi_patch_nhatf {
    const double *patch_weights_dev;          /* coupled patch, or NULL */
    const double *grad_dev[3];                /* coupled: the cell gradient; otherwise the boundary value of gradAlpha per patch face */
    const double *nbr_grad_dev[3];            /* coupled only */
    const double *patch_sf_dev[3];
    const double *patch_magsf_dev;            /* contact-angle form */
    const double *theta_deg_dev;              /* contact-angle form, degrees per face; NULL otherwise */
    double *nhatf_out_dev;
    double *nhatfv_out_dev[3];                /* all three or all NULL */
    double *gradient_out_dev;                 /* contact-angle form, or NULL */
    double *b1_out_dev, *b2_out_dev;          /* contact-angle form, both or neither */
} mi_patch_nhatf;
typedef struct mi_interface_s *mi_interface_t;
int mi_interface_nhatf(mi_addr_t addr, double delta_n, const double *lambda_dev, const double *const *sf_dev, const double *const *grad_dev,
                       double *nhatf_out_dev, double *const *nhatfv_out_dev_or_null);
int mi_patch_interface_nhatf(mi_patch_t patch, double delta_n, const mi_patch_nhatf *arrays);
int mi_interface_create(mi_addr_t addr, mi_grad_boundary_t boundary_or_null, mi_interface_t *out);
int mi_interface_destroy(mi_interface_t iface);
int mi_interface_curvature(mi_interface_t iface, const double *nhatf_dev, const double *b_nhatf_dev, const double *vol_dev, double *k_out_dev);
int mi_surface_tension_force(mi_addr_t addr, double sigma, const double *lambda_dev, const double *delta_coeffs_dev, const double *k_dev,
                             const double *alpha_dev, const double *sngrad_corr_dev_or_null, double *out_dev);
int mi_patch_surface_tension_force(mi_patch_t patch, double sigma, const double *patch_weights_dev, const double *patch_delta_coeffs_dev,
                                   const double *k_dev, const double *nbr_k_dev, const double *alpha_dev, const double *nbr_alpha_dev,
                                   const double *patch_sngrad_corr_dev_or_null, double *out_dev);
int mi_near_interface(mi_ctx_t ctx, int64_t n, const double *alpha_dev, double *out_dev);
/* ---- the kEpsilon turbulence model: G, the wall functions, bound and nut (turbulenceModels/incompressible/RAS/kEpsilon/kEpsilon.C:132-136,
 *      :229-280; epsilonWallFunctionFvPatchScalarField.C:116-396, :540-589; nutkWallFunctionFvPatchScalarField.C:60-77; bound.C:32-60;
 *      fvcAverage.C:71-74) ----
 * What incompressible::RASModels::kEpsilon::correct() runs as about forty field passes is eight kernels of this block, four mi_min_max
 * reductions for the two bound decisions and three launches per bound that has to act, beside the assembly, relaxation, setValues, solve
 * and boundary evaluation of every transport equation (DESIGN 3.5o counts them).  All values are fp64, all labels int32.  Every operator is rounded on its own except the fma written below; division and
 * square root are the correctly rounded IEEE ones; max(a, b) = (a > b) ? a : b and pos(x) = (x >= 0) ? 1 : 0 throughout.  A cell meets its
 * faces in the order of mi_surface_sum / mi_interface_curvature: own faces ascending, neighbour-side faces in losort order, boundary faces
 * patch by patch.  Restated in tests/turbulence_support.py, not pinned by a compiled reference.
 * mi_ke_coeffs_init (host only, no GPU): Cmu25 = sqrt(sqrt(Cmu)) (pow025), Cmu75 = pow(Cmu, 0.75), yPlusLam = ten iterations of
 *   ypl = log(max(E*ypl, 1))/kappa from 11.0 (nutWallFunctionFvPatchScalarField.C:154-167) with the host's libm.  The reference's defaults are
 *   0.09, 1.44, 1.92, 1.3, 0.41, 9.8.  An entry that takes a mi_ke_coeffs refuses one with a non-finite or non-positive member.
 * mi_min_max: the smallest and the largest of n values to the host (either output may be NULL): what bound's test (bound.C:35-37) and a
 *   Courant number need.  Order-independent, hence exact; n == 0 gives +inf / -inf.  The inputs are assumed finite: the result for a NaN
 *   among them is unspecified, and so is the sign of a zero result when both zeros occur.  Synchronises the context's stream.
 * mi_vec_max_value: out = max(x, value); out may be x.  The boundary line of bound (:56).
 * mi_average_create / mi_average_destroy: the handle of fvc::average on one mesh: it keeps surfaceSum(magSf) per cell and one scratch cell
 *   array.  boundary NULL: no boundary faces; otherwise it must outlive the handle.  mag_sf_dev: internal faces; b_mag_sf_dev: the
 *   patch-ordered boundary faces of `boundary`.  After mesh motion: destroy and create.
 * mi_fvc_average: out = surfaceSum(magSf*ssf)/surfaceSum(magSf): each product rounded, then added in the order above; one division per
 *   cell; one row pass.  A cell without faces gives 0/0.
 * mi_bound: bound.C:45-54 for the internal field in ONE row pass that writes no face field.  Per face, with m = max(v, lb) on both sides,
 *   i = fma(lambda, mP - mN, mN) (the rule of mi_face_interpolate); avg as mi_fvc_average forms it, the boundary faces taking b_face_dev;
 *   then v = max(max(v, avg*pos(-v)), lb).  b_face_dev: the patch-ordered boundary values of linearInterpolate(max(vsf, lb)), the caller's:
 *   mi_vec_max_value on the boundary values, and on coupled patches w*mP + (1 - w)*mNbr.  A cell reads its neighbours' OLD values: the pass
 *   writes the handle's scratch array and copies it back, so the result has the bits of the out-of-place sequence mi_vec_max_value +
 *   mi_face_interpolate + mi_fvc_average + the cell algebra.  Whether to bound at all (min(vsf) < lb, :35-37) is the caller's decision, made
 *   with mi_min_max on the internal and the boundary values.
 * mi_ke_production (:238): G = (nut*2)*magSqr(symm(gradU)) in one cell pass over grad_dev[3*j + k] = d(U_j)/dx_k, the nine arrays of
 *   mi_limited_grad's layout.  symm: xy = 0.5*(g_xy + g_yx), likewise xz and yz.  magSqr (SymmTensorI.H:276-284), left to right:
 *     s = fma(xx, xx, 2*(xy*xy)); s = fma(2, xz*xz, s); s = fma(yy, yy, s); s = fma(2, yz*yz, s); s = fma(zz, zz, s)
 *   -- the squares of the diagonal contracted into the running sum, the doubled squares rounded first (doubling is exact, so fma(2, q, s)
 *   is s + 2*q): an ASSUMPTION, see DESIGN 3.5o.  (nut*2)*s equals nut*(2*s): doubling is exact.
 * mi_ke_create / mi_ke_destroy: the wall cells of one mesh, built once on the host from `boundary` and patch_is_wall[p] != 0 per patch: the
 *   union of the cells of the flagged patches, ascending; per such cell its wall faces by patch, then by face; cornerWeight =
 *   1.0/(wall faces of the cell) (epsilonWallFunctionFvPatchScalarField.C:146-200).  The boundary must outlive the handle.
 * mi_ke_wall_cells (:241): epsilon.boundaryField().updateCoeffs() for ALL wall patches in ONE launch, no atomics.  Every b_* array of
 *   mi_ke_wall is patch-ordered over `boundary`; only wall faces are read or written.  Per unique wall cell c, Gc and ec start at 0.0 and its
 *   wall faces are visited in (patch, face) order:
 *     sn_k = dc*(Uw_k - U_k[c]);  mgu = sqrt(fma(sn_z, sn_z, fma(sn_x, sn_x, sn_y*sn_y)))     (mag: the contraction of 3.5a, an assumption)
 *     ec += ((w*Cmu75)*pow(k[c], 1.5))/(kappa*y)
 *     Gc += ((((w*(nutw + nuw))*mgu)*Cmu25)*sqrt(k[c]))/(kappa*y)
 *   then g_inout[c] = Gc, eps_inout[c] = ec and b_eps_out[face] = ec for each of the cell's wall faces (the zero-gradient assignment
 *   :245-253).  Cells that are not wall cells keep their G and epsilon.  pow is the device library's fp64 pow, evaluated once per cell;
 *   b_pow_out_dev, when given, receives it per wall face (for tests).
 * mi_ke_wall_cell_labels: the unique wall cells on the device, ascending; boundaryManipulate (:255) is mi_fvm_set_values with them and with
 *   the values mi_ke_wall_values gathers (values_out[i] = eps[label[i]]).
 * mi_ke_epsilon_terms (:250-251, DepsilonEff): su = ((C1*G)*eps)/k, sp = (C2*eps)/k, deps = nut/sigmaEps + nu in one cell pass; nu a cell
 *   array, or nu_value when nu_dev_or_null is NULL.  mi_ke_k_terms (:269, DkEff): sp = eps/k, dk = nut + nu.  su and sp are what
 *   mi_fvm_assemble takes as su_dev and sp_dev; deps / dk go through mi_face_interpolate into mi_fvm_laplacian's gammaMagSf; G itself is
 *   the su of the k equation.
 * mi_ke_nut (:135, :278): nut = (Cmu*(k*k))/eps.  mi_ke_nut_wall: nutkWallFunction::calcNut on every wall face in one launch:
 *   yPlus = ((Cmu25*y)*sqrt(k[c]))/nuw; yPlus > yPlusLam: nutw = nuw*(((yPlus*kappa)/log(E*yPlus)) - 1.0); otherwise exactly 0.
 *   b_log_out_dev_or_null receives the device library's log where the branch is taken and is not written elsewhere (for tests).
 *   kqRWallFunction is zero-gradient: mi_patch_internal_field.
 * The cell passes take two cells per thread with 16-byte accesses when every array is 16-byte aligned, one by one otherwise; they and the
 *   wall passes run under the context's launch-grid cap (MI_FACE_GRID).
 * Refused (MI_ERR_ARG, nothing launched, nothing written): missing arrays; an output that aliases an input or another output (except
 *   mi_vec_max_value's out and mi_bound's vsf_inout); an array not aligned for a double; a handle or boundary of another addressing; NULL
 *   boundary arrays while the boundary has faces; patch_is_wall flagging a coupled patch; a coefficient that is not finite or not above zero;
 *   a lower bound that is not a number.
 *   mi_min_max during a PCG session: MI_ERR_STATE.  Zero cells, zero wall faces and zero wall patches: MI_OK.
 * Out of scope: the wall-distance field itself (wallDist / meshWave: kOmegaSST, below, takes y as the caller's cell array); the low-Re and rough wall functions;
 *   the nutU* wall functions (nutUSpalding: the Spalart-Allmaras block); the weighted (weights) forms of the epsilon wall function; compressible kEpsilon (rho-weighted);
 *   a pisoFoam / simpleFoam application; moving meshes; nearWallDist (y is the caller's patch array). */
typedef struct mi_ke_coeffs {
    double Cmu, C1, C2, sigmaEps, kappa, E;
    double Cmu25, Cmu75, yPlusLam;            /* derived: mi_ke_coeffs_init */
} mi_ke_coeffs;
typedef struct mi_ke_wall {
    const double *k_dev;
    const double *u_dev[3];
    const double *b_uw_dev[3];                /* the boundary face values of U */
    const double *b_delta_coeffs_dev, *b_y_dev, *b_nuw_dev, *b_nutw_dev;
    double *g_inout_dev, *eps_inout_dev;      /* cell fields: the wall cells are overwritten */
    double *b_eps_out_dev;
    double *b_pow_out_dev;                    /* or NULL */
} mi_ke_wall;
typedef struct mi_average_s *mi_average_t;
typedef struct mi_ke_s *mi_ke_t;
int mi_ke_coeffs_init(double Cmu, double C1, double C2, double sigmaEps, double kappa, double E, mi_ke_coeffs *out);
int mi_min_max(mi_ctx_t ctx, int64_t n, const double *x_dev, double *min_out_host, double *max_out_host);
int mi_vec_max_value(mi_ctx_t ctx, int64_t n, const double *x_dev, double value, double *out_dev);
int mi_average_create(mi_addr_t addr, mi_grad_boundary_t boundary_or_null, const double *mag_sf_dev, const double *b_mag_sf_dev, mi_average_t *out);
int mi_average_destroy(mi_average_t average);
int mi_fvc_average(mi_average_t average, const double *mag_sf_dev, const double *b_mag_sf_dev, const double *ssf_dev, const double *b_ssf_dev,
                   double *out_dev);
int mi_bound(mi_average_t average, double lower_bound, const double *lambda_dev, const double *mag_sf_dev, const double *b_mag_sf_dev,
             const double *b_face_dev, double *vsf_inout_dev);
int mi_ke_production(mi_ctx_t ctx, int64_t n, const double *nut_dev, const double *const *grad_dev, double *g_out_dev);
int mi_ke_create(mi_addr_t addr, mi_grad_boundary_t boundary, const int32_t *patch_is_wall, mi_ke_t *out);
int mi_ke_destroy(mi_ke_t ke);
int mi_ke_wall_cells(mi_ke_t ke, const mi_ke_coeffs *coeffs, const mi_ke_wall *arrays);
int mi_ke_wall_cell_labels(mi_ke_t ke, int32_t *n_out, const int32_t **labels_dev_out);
int mi_ke_wall_values(mi_ke_t ke, const double *eps_dev, double *values_out_dev);
int mi_ke_epsilon_terms(mi_ctx_t ctx, int64_t n, const mi_ke_coeffs *coeffs, const double *g_dev, const double *eps_dev, const double *k_dev,
                        const double *nut_dev, const double *nu_dev_or_null, double nu_value, double *su_out_dev, double *sp_out_dev,
                        double *deps_out_dev);
int mi_ke_k_terms(mi_ctx_t ctx, int64_t n, const double *eps_dev, const double *k_dev, const double *nut_dev, const double *nu_dev_or_null,
                  double nu_value, double *sp_out_dev, double *dk_out_dev);
int mi_ke_nut(mi_ctx_t ctx, int64_t n, double Cmu, const double *k_dev, const double *eps_dev, double *nut_out_dev);
int mi_ke_nut_wall(mi_ke_t ke, const mi_ke_coeffs *coeffs, const double *k_dev, const double *b_y_dev, const double *b_nuw_dev,
                   double *b_nutw_out_dev, double *b_log_out_dev_or_null);
/* ---- the kOmegaSST turbulence model: blending, the omega wall function, sources and nut (turbulenceModels/incompressible/RAS/kOmegaSST/
 *      kOmegaSST.C:47-111, :127-243, :284-296, :398-468; kOmegaSST.H:164-243; omegaWallFunctionFvPatchScalarField.C:209-239, :241-394,
 *      :548-596; fvMatrix.C:2208-2216, :2759-2814; fvmSup.C:100-214) ----
 * What incompressible::RASModels::kOmegaSST::correct() runs as about sixty field passes is six kernels of this block and two or three of the
 * kEpsilon block (mi_ke_wall_values, mi_ke_nut_wall, the bound decisions), beside the gradients, the assembly, relaxation, setValues, solve
 * and boundary evaluation of both transport equations (DESIGN 3.5p counts them).  The rules of the kEpsilon block hold: fp64 values, int32
 * labels, every operator rounded on its own except the fma written below, correctly rounded division and square root,
 * max(a, b) = (a > b) ? a : b, min(a, b) = (a < b) ? a : b (doubleFloat.H), pow4(s) = sqr(sqr(s)) (Scalar.H:189).  tanh is the device
 * library's and NOT the reference's bits: F1 and F23 are outputs, and everything formed from them is exact given them.  y, the distance of
 * every cell centre to the nearest wall (wallDist, :245, :409), is the caller's cell array; b_y of the wall faces (nearWallDist) the caller's
 * patch array, as for kEpsilon.  Restated in tests/komegasst_support.py, not pinned by a compiled reference.
 * mi_sst_coeffs_init (host only, no GPU): model_or_null = {alphaK1, alphaK2, alphaOmega1, alphaOmega2, gamma1, gamma2, beta1, beta2, betaStar,
 *   a1, b1, c1}, NULL for the reference's defaults 0.85, 1.0, 0.5, 0.856, 5.0/9.0, 0.44, 0.075, 0.0828, 0.09, 0.31, 1.0, 10.0 (:127-243);
 *   wall_or_null = {Cmu, kappa, E, beta1} of the omega wall function, NULL for 0.09, 0.41, 9.8, 0.075 (:406-409).  The products of
 *   dimensionedScalars are formed once, in the reference's order: twoAlphaOmega2 = 2*alphaOmega2 (:420), fourAlphaOmega2 = 4*alphaOmega2 (:64),
 *   invBetaStar = 1/betaStar (:61), twoInvBetaStar = 2/betaStar (:80), c1a1BetaStar = (c1/a1)*betaStar (:433), c1BetaStar = c1*betaStar (:456),
 *   d<X> = X1 - X2 of blend (kOmegaSST.H:171); Cmu25 and yPlusLam as mi_ke_coeffs_init forms them.  An entry that takes a mi_sst_coeffs refuses
 *   one whose members are not all finite and (the differences apart) above zero.
 * mi_sst_production (:412-413): S2 = 2*magSqr(symm(gradU)), G = nut*S2 in one cell pass; magSqr(symm) is mi_ke_production's (one device
 *   function), so G has the bits of mi_ke_production's (nut*2)*magSqr.  mag_out_dev_or_null receives mag(symm(gradU)) = sqrt(magSqr) for the
 *   constructor's form of nut (:287-295).
 * mi_sst_wall_cells (:416): omega.boundaryField().updateCoeffs() for ALL wall patches in ONE launch on a mi_ke_t, no atomics, as
 *   mi_ke_wall_cells: per unique wall cell c, from 0.0, its wall faces in (patch, face) order (calculateTurbulenceFields :209-239):
 *     omegaVis = (6.0*nuw)/(beta1*sqr(y));  omegaLog = sqrt(k[c])/((Cmu25*kappa)*y)                  (OmegaCalculateOmegaFunctor :270-279)
 *     oc += w*sqrt(fma(omegaVis, omegaVis, omegaLog*omegaLog))      (the first square contracted into the sum: an ASSUMPTION)
 *     Gc += ((((w*(nutw + nuw))*mgu)*Cmu25)*sqrt(k[c]))/(kappa*y)   (OmegaCalculateGFunctor :315-325; mgu as in mi_ke_wall_cells)
 *   then g_inout[c] = Gc, omega_inout[c] = oc (:580-586) and b_omega_out[face] = oc (:227-237).  No transcendental: the reference's bits.
 *   boundaryManipulate (:444) is mi_fvm_set_values with mi_ke_wall_cell_labels and mi_ke_wall_values.
 * mi_sst_blend (:418-439, F1 :47-70, F23 :73-111, blend / DkEff / DomegaEff kOmegaSST.H:164-243): one cell pass.
 *     CDkOmega = (twoAlphaOmega2*fma(gKz, gOz, fma(gKx, gOx, gKy*gOy)))/omega                        (the dot product of 3.5a)
 *     arg1 = min(min(max((invBetaStar*sqrt(k))/(omega*y), (500*nu)/(sqr(y)*omega)), (fourAlphaOmega2*k)/(max(CDkOmega, 1e-10)*sqr(y))), 10)
 *     F1 = tanh(pow4(arg1));  arg2 = min(max((twoInvBetaStar*sqrt(k))/(omega*y), (500*nu)/(sqr(y)*omega)), 100);  F2 = tanh(sqr(arg2))
 *     f3 != 0: arg3 = min((150*nu)/(omega*sqr(y)), 10), F23 = F2*(1 - tanh(pow4(arg3))); otherwise F23 = F2
 *     blend(X) = F1*dX + X2
 *     su = blend(gamma)*min(S2, (c1a1BetaStar*omega)*max(a1*omega, (b1*F23)*sqrt(S2)));  sp = blend(beta)*omega
 *     susp = ((F1 - 1)*CDkOmega)/omega;  DomegaEff = blend(alphaOmega)*nut + nu;  DkEff = blend(alphaK)*nut + nu
 *   nu a cell array, or nu_value when nu_dev_or_null is NULL.  The optional outputs (for tests) are CDkOmega and arg1 -- the reference's
 *   bits, no transcendental comes before them -- F23 and tanh(pow4(arg3)) (0 when f3 == 0).
 * mi_sst_omega_sources (:432-439): the right-hand side su - fvm::Sp(sp, omega) - fvm::SuSp(susp, omega) is a matrix of its own in the
 *   reference, built as (su - Sp) - SuSp -- operator-(su, A) negates A and subtracts V*su from its source (fvMatrix.C:2759-2814), operator-=
 *   subtracts diagonals and sources (:1787-1795), SuSp is diag = V*max(susp, 0), source = 0 - (V*min(susp, 0))*omega (fvmSup.C:194-214) --
 *   and operator== subtracts it from the left side (:2208-2216).  In place on what mi_fvm_assemble wrote for ddt + div - laplacian:
 *     diag   = diag   - ((-(V*sp)) - V*max(susp, 0))
 *     source = source - ((-(V*su)) - (0 - (V*min(susp, 0))*omega))
 *   The two implicit parts meet each other BEFORE the left side's diagonal: not the bits of mi_fvm_sp followed by mi_fvm_susp.
 * mi_sst_k_terms (:456-457): su = min(G, (c1BetaStar*k)*omega), sp = betaStar*omega with the NEW omega; they go into mi_fvm_assemble as
 *   su_dev and sp_dev, which gives the bits of the reference's su - fvm::Sp for a single implicit part.
 * mi_sst_nut (:466; constructor_form != 0: :287-295): nut = (a1*k)/max(a1*omega, (b1*F23)*sqrt(S2)) with F23 recomputed in the pass from k,
 *   omega, y and nu; the constructor's form takes s_dev = mag(symm(gradU)) and forms ((b1*F23)*sqrt(2.0))*s.  On the boundary values of
 *   non-wall patches the same entry on boundary arrays; wall patches are mi_ke_nut_wall.
 * Refused (MI_ERR_ARG, nothing launched, nothing written): as in the kEpsilon block -- missing arrays, an output that aliases an input or
 *   another output (mi_sst_omega_sources's diag and source are in-out), an array not aligned for a double, a handle of another addressing,
 *   coefficients that are not finite or not above zero, a nu_value that is not.  Zero cells and zero wall faces: MI_OK.
 * Out of scope: wallDist / meshWave; the weighted (weights) omega wall function; the low-Re, rough and nutU* wall functions (nutUSpalding: the Spalart-Allmaras block); kOmega,
 *   kOmegaSSTSAS; compressible kOmegaSST; coupled wall patches; moving meshes; a simpleFoam / pisoFoam application. */
typedef struct mi_sst_coeffs {
    double alphaK1, alphaK2, alphaOmega1, alphaOmega2, gamma1, gamma2, beta1, beta2, betaStar, a1, b1, c1;
    double Cmu, kappa, E, wallBeta1;          /* the omega wall function's */
    double twoAlphaOmega2, fourAlphaOmega2, invBetaStar, twoInvBetaStar, c1a1BetaStar, c1BetaStar;   /* derived: mi_sst_coeffs_init */
    double dAlphaK, dAlphaOmega, dBeta, dGamma;
    double Cmu25, yPlusLam;
} mi_sst_coeffs;
typedef struct mi_sst_wall {
    const double *k_dev;
    const double *u_dev[3];
    const double *b_uw_dev[3];                /* the boundary face values of U */
    const double *b_delta_coeffs_dev, *b_y_dev, *b_nuw_dev, *b_nutw_dev;
    double *g_inout_dev, *omega_inout_dev;    /* cell fields: the wall cells are overwritten */
    double *b_omega_out_dev;
} mi_sst_wall;
typedef struct mi_sst_blend_arrays {
    const double *grad_k_dev[3], *grad_omega_dev[3];
    const double *k_dev, *omega_dev, *y_dev, *nut_dev, *s2_dev;
    const double *nu_dev_or_null;
    double nu_value;
    double *f1_out_dev, *su_out_dev, *sp_out_dev, *susp_out_dev, *domega_out_dev, *dk_out_dev;
    double *cdkomega_out_dev_or_null, *arg1_out_dev_or_null, *f23_out_dev_or_null, *tanh3_out_dev_or_null;
} mi_sst_blend_arrays;
int mi_sst_coeffs_init(const double *model_or_null, const double *wall_or_null, mi_sst_coeffs *out);
int mi_sst_production(mi_ctx_t ctx, int64_t n, const double *nut_dev, const double *const *grad_dev, double *s2_out_dev, double *g_out_dev,
                      double *mag_out_dev_or_null);
int mi_sst_wall_cells(mi_ke_t ke, const mi_sst_coeffs *coeffs, const mi_sst_wall *arrays);
int mi_sst_blend(mi_ctx_t ctx, int64_t n, const mi_sst_coeffs *coeffs, int f3, const mi_sst_blend_arrays *arrays);
int mi_sst_omega_sources(mi_ctx_t ctx, int64_t n, const double *vol_dev, const double *su_dev, const double *sp_dev, const double *susp_dev,
                         const double *omega_dev, double *diag_inout_dev, double *source_inout_dev);
int mi_sst_k_terms(mi_ctx_t ctx, int64_t n, const mi_sst_coeffs *coeffs, const double *g_dev, const double *k_dev, const double *omega_dev,
                   double *su_out_dev, double *sp_out_dev);
int mi_sst_nut(mi_ctx_t ctx, int64_t n, const mi_sst_coeffs *coeffs, int f3, int constructor_form, const double *k_dev, const double *omega_dev,
               const double *y_dev, const double *s_dev, const double *nu_dev_or_null, double nu_value, double *nut_out_dev,
               double *f23_out_dev_or_null);
/* ---- the thermo update of rhoPimpleFoam: T from he, psi, mu, alpha, rho (thermophysicalModels/basic/psiThermo/hePsiThermo.C:31-171,
 *      rhoThermo/heRhoThermo.C:31-177, heThermo/heThermo.C:131-145, :397-760, :875-960; specie/thermo/thermo/thermoI.H:42-90 and below;
 *      hConst/hConstThermoI.H:93-140, eConst/eConstThermoI.H:94-143, janaf/janafThermoI.H:58-71, :119-141, :188-241, janafThermo.C:31-53;
 *      equationOfState/perfectGas/perfectGasI.H:80-106; transport/const/constTransportI.H:98-128, sutherland/sutherlandTransportI.H:133-164;
 *      DESIGN 3.5q) ----
 * thermo.correct() (rhoPimpleFoam/EEqn.H:31) is hePsiThermo::calculate(): per cell and per patch face a Newton iteration for T from he and
 * p, then psi, mu and alpha; heRhoThermo::calculate() adds rho.  One pure mixture of one thermoType:
 *   energy         sensibleEnthalpy (he = Hs, Cpv = Cp, THE = THs) | sensibleInternalEnergy (he = Es, Cpv = Cv, THE = TEs)
 *   thermodynamics hConst {Cp, Hf} | eConst {Cv, Hf} | janaf {Tlow, Thigh, Tcommon, highCpCoeffs[7], lowCpCoeffs[7]}
 *   equation of state  perfectGas {W}: rho = p/(R*T), psi = 1.0/(R*T), cpMcv = 8314.4621, R = 8314.4621/W
 *   transport      const {mu, Pr} | sutherland {As, Ts}
 * The rules of the kEpsilon block hold: fp64 values, int32 labels, every operator rounded on its own except the fma written below, correctly
 * rounded division and square root, max(a, b) = (a > b) ? a : b, min(a, b) = (a < b) ? a : b (doubleFloat.H), mag = fabs.  No transcendental
 * function is called, so given the contraction below every output is the reference's bit for bit.  Restated in tests/thermo_support.py, not
 * pinned by a compiled reference.
 * mi_thermo_model_init (host only, no GPU): thermo_values = {Cp, Hf} | {Cv, Hf} | {Tlow, Thigh, Tcommon, high[7], low[7]} and
 *   transport_values = {mu, Pr} | {As, Ts}, the dictionary's per-mass numbers.  Formed once, in the constructors' order: R = 8314.4621/W,
 *   CpW = Cp*W, CvW = Cv*W, HfW = Hf*W (hConstThermo.C:40-41, eConstThermo.C likewise; janafThermo.C scales nothing), cpE = CvW + cpMcv
 *   (eConstThermoI.H:111), rPr = 1.0/Pr (constTransport.C:47); for janaf the quotients {a1/2.0, a2/3.0, a3/4.0, a4/5.0} of each set
 *   (highH, lowH) and hc = 8314.4621*fma(fma(fma(fma(fma(l4/5, Tstd, l3/4), Tstd, l2/3), Tstd, l1/2), Tstd, l0), Tstd, l5), Tstd = 298.15, of
 *   the LOW set (janafThermoI.H:230-241).  Refused: a member that is not finite, or not above zero -- Hf and the janaf coefficients may
 *   have any finite sign -- and what janafThermo::checkInputData refuses: Tlow >= Thigh, Tcommon <= Tlow, Tcommon > Thigh.  Members of the
 *   parts not chosen stay 0 and are not looked at.  An entry that takes a model refuses one that init would refuse.
 * The formulas (cp, hs per kmol; W the molecular weight):
 *     hConst: cp = CpW, hs = CpW*T.   eConst: cp = cpE, hs = cpE*T.
 *     janaf: a = (T < Tcommon) ? low : high at EVERY evaluation;  cp = 8314.4621*fma(fma(fma(fma(a4, T, a3), T, a2), T, a1), T, a0);
 *            hs = ha - hc = fma(8314.4621, fma(fma(fma(fma(fma(a4/5.0, T, a3/4.0), T, a2/3.0), T, a1/2.0), T, a0), T, a5), -hc)
 *     Hs = hs/W;  Cp = cp/W;  Cv = cv/W with cv = cp - cpMcv, for janaf cv = fma(8314.4621, chain of cp, -cpMcv): cp's product has this one
 *            use and contracts with the subtraction (the Newton divisor of the internal energy, sutherland's Cv_, the Cv / Cpv / kappa
 *            properties all take it);  Es = es/W with q = (p*W)/rho(p, T) and
 *            es = fma(CpW, T, -q) (hConst) | fma(cpE, T, -q) (eConst) | hs - q (janaf: hs ends in an fma already)
 *     gamma = cp/(cp - cpMcv) with cp ROUNDED, janaf included: the product has two uses there (thermoI.H:148-149) and stays a product;
 *            CpByCpv = 1 (enthalpy) | gamma (internal energy)
 *     const: mu = mu_, alphah = mu_*rPr, kappa = (Cpv*mu_)*rPr.
 *     sutherland: mu = (As*sqrt(T))/(1.0 + Ts/T), kappa = (mu*Cv_)*(1.32 + (1.77*R)/Cv_) with Cv_ = Cv(p, T), alphah = kappa/Cpv
 *   Rounded first, NOT contracted: Cv_ + cpMcv, 1.32 + (1.77*R)/Cv_, the Newton update (a division stands before each sum), hConst's and
 *   eConst's hs of the enthalpy form.  The fma above are what the x86 compiler's contraction (-ffp-contract=fast) makes of the reference's
 *   expressions, taken for nvcc's: an ASSUMPTION.
 * The Newton iteration is thermo::T (thermoI.H:42-90): Ttol = T0*1.0e-4; do { Test = Tnew; Tnew = limit(Test - (F(p, Test) - f)/dFdT(p, Test));
 *   if (iter++ > 100) return NaN; } while (mag(Tnew - Test) > Ttol) -- the NaN of the reference's device branch (0.0/0.0), on the 102nd
 *   evaluation.  F / dFdT = Hs / Cp or Es / Cv.  limit is the identity for hConst / eConst and, for janaf, min(max(T, Tlow), Thigh) when
 *   T < Tlow || T > Thigh (janafThermoI.H:119-141).
 * mi_thermo_calculate: hePsiThermoCalculateFunctor / heRhoThermoCalculateFunctor on n elements in one launch: T = THE(he, p, T0), psi, mu,
 *   alpha at the new T; 24 bytes in, 32 out, 40 with rho.  rho_form 0: no rho; 1: rho = p/(R*T), heRhoThermo's mixture.rho; 2: rho = psi*p,
 *   psiThermo::rho(), what rhoPimpleFoam assigns after correct().  t_out may be t0 itself (the normal in-place use) or he itself (fault 1
 *   below); every element is read before it is written; any other overlap of an output with an input or an output is refused.
 *   iters_out_or_null (int32, for the tests) receives the number of evaluations of the Newton step.  Two cells per thread with 16-byte
 *   accesses when every double array is 16-byte aligned, one by one otherwise; under the context's launch-grid cap (MI_FACE_GRID).  The
 *   model travels by value in the kernel arguments; janaf's coefficient sets (and the boundary pass's run table) are staged in LDS.
 * mi_thermo_calculate_boundary: the patch loop of hePsiThermo.C:109-171 / heRhoThermo.C:111-177 for ALL patches in ONE launch (one per 16 runs
 *   of consecutive patches of one kind) over the patch-ordered boundary arrays of a mi_grad_boundary_t.  patch_kind[p] = 0: skip (empty);
 *   1: fixesValue(): b_he = HE(p, T), the properties at the given T; 2: b_t_out = THE(he, p, T), the properties at the new T.
 * mi_thermo_he: he = HE(p, T) on n elements: heThermo::init() on the cells, and he(p, T, patchi) on a patch -- the caller passes the patch's
 *   slice of its boundary arrays (no patch mask).
 * mi_thermo_property: one of MI_THERMO_CP / CV / GAMMA / CPV / CPBYCPV / KAPPA from p and T, cells or a patch slice: the mixture's members that
 *   heThermo.C:397-760 transforms over.  MI_THERMO_KAPPA is the TRANSPORT model's kappa(p, T) (constTransportI.H:110-117,
 *   sutherlandTransportI.H:145-152), NOT heThermo::kappa(): that one is Cp()*alpha_ (heThermo.C:875-896), kappaEff is Cp*alphaEff(alphat) and
 *   alphaEff is CpByCpv*(alpha_ + alphat) (:901-962) -- products of fields: MI_THERMO_CP or MI_THERMO_CPBYCPV, then the caller's field
 *   product with alpha or with alpha + alphat (mi_vec_axpby forms the sum).
 * Two faults of the reference, decided here:
 *   1. On a patch that does not fix T the reference's transform writes the new temperature into the he patch field -- its output tuple starts
 *      with ph.begin() (hePsiThermo.C:161-169, heRhoThermo.C:166-175) -- and pT stays as it was; the loop it replaced, still in the comment
 *      above it, assigns pT[facei].  Here the outputs are the caller's pointers: b_t_out = b_t is OpenFOAM's meaning (the default of the Python
 *      binding and the mirror), b_t_out = b_he reproduces the reference's transform.
 *   2. On a fixesValue patch heRhoThermo's functor returns psi in the rho slot (heRhoThermo.C:57-61).  Here rho(p, T) is written (by
 *      rho_form).  A caller who wants the reference's bits runs rho_form 0 on those patches' behalf and copies b_psi.
 * Refused (MI_ERR_ARG, nothing launched, nothing written): a missing array; an array not aligned for a double, iters not for an int32; an
 *   overlap other than the two allowed; an unknown energy form, thermodynamics, transport, rho_form, property kind or patch kind; a boundary
 *   of another addressing; NULL boundary arrays while a patch of kind 1 or 2 has faces; a model init would refuse; rho_form != 0 with no rho
 *   array.  Zero elements, zero patches and patches all of kind 0: MI_OK without a launch.
 * Out of scope: mixtures of several species, reacting thermo, the other equations of state, hPolynomial / polynomialTransport /
 *   hExponential, absolute enthalpy / internal energy, heBoundaryCorrection, psi.oldTime(), compressible turbulence, moving meshes. */
enum { MI_THERMO_ENTHALPY = 0, MI_THERMO_INTERNAL_ENERGY = 1 };
enum { MI_THERMO_HCONST = 0, MI_THERMO_ECONST = 1, MI_THERMO_JANAF = 2 };
enum { MI_THERMO_CONST = 0, MI_THERMO_SUTHERLAND = 1 };
enum { MI_THERMO_CP = 0, MI_THERMO_CV = 1, MI_THERMO_GAMMA = 2, MI_THERMO_CPV = 3, MI_THERMO_CPBYCPV = 4, MI_THERMO_KAPPA = 5 };
typedef struct mi_thermo_model {
    int32_t energy, thermo, transport, reserved;
    double W;
    double Cp, Cv, Hf;                        /* hConst: Cp, Hf; eConst: Cv, Hf (per mass, as given) */
    double Tlow, Thigh, Tcommon, highCpCoeffs[7], lowCpCoeffs[7];   /* janaf */
    double mu, Pr, As, Ts;                    /* const: mu, Pr; sutherland: As, Ts */
    double R, cpMcv, CpW, CvW, HfW, cpE, rPr; /* derived: mi_thermo_model_init */
    double highH[4], lowH[4], hc;
} mi_thermo_model;
int mi_thermo_model_init(int energy, int thermo, int transport, double W, const double *thermo_values, const double *transport_values,
                         mi_thermo_model *out);
int mi_thermo_calculate(mi_ctx_t ctx, const mi_thermo_model *model, int rho_form, int64_t n, const double *he_dev, const double *p_dev,
                        const double *t0_dev, double *t_out_dev, double *psi_out_dev, double *mu_out_dev, double *alpha_out_dev,
                        double *rho_out_dev_or_null, int32_t *iters_out_or_null);
int mi_thermo_calculate_boundary(mi_addr_t addr, mi_grad_boundary_t boundary, const mi_thermo_model *model, const int32_t *patch_kind,
                                 int rho_form, double *b_he_inout_dev, const double *b_p_dev, const double *b_t_dev, double *b_t_out_dev,
                                 double *b_psi_out_dev, double *b_mu_out_dev, double *b_alpha_out_dev, double *b_rho_out_dev_or_null);
int mi_thermo_he(mi_ctx_t ctx, const mi_thermo_model *model, int64_t n, const double *p_dev, const double *t_dev, double *he_out_dev);
int mi_thermo_property(mi_ctx_t ctx, const mi_thermo_model *model, int kind, int64_t n, const double *p_dev, const double *t_dev,
                       double *out_dev);
/* ---- rhoCentralFoam's Kurganov and Tadmor face fluxes (applications/solvers/compressible/rhoCentralFoam/rhoCentralFoam.C:60-185,
 *      readFluxScheme.H, createFields.H:76-98, compressibleCourantNo.H:35-47) ----
 * What the top of rhoCentralFoam's time loop runs as ten limited interpolations and about forty-five face-field operators (some seventy
 * passes with face-sized temporaries) is ONE face pass here, with a patch form, one cell pass and one reduction beside it.
 * mi_central_scheme_parse: host only.  flux_scheme "Kurganov" | "Tadmor" (readFluxScheme.H), anything else MI_ERR_ARG.  The three
 *   reconstruct(...) entries go through mi_limiter_parse unchanged: every TVD/NVD name it accepts is accepted.  reconstruct(rho) and
 *   reconstruct(T) limit scalars (the bounded forms allowed, a V form refused); reconstruct(U) may be a V form, limited on rhoU itself, or a
 *   scalar form, limited on the caller's magSqr(rhoU) and its gradient (LimitFuncs.C:39-54, as mi_limited_weights).  Refused with *out
 *   untouched: the filtered names and whatever mi_limiter_parse refuses.
 * mi_central_flux (internal faces; :62-185): with P = lower[f], N = upper[f], d = C[N] - C[P], per field v of rho, rhoU, rPsi, e, c (under
 *   reconstruct(rho), (U), (T), (T), (T)) and per direction, pos with faceFlux fl = +1.0 and neg with fl = -1.0 (createFields.H:76-98):
 *     lim = the limiter of mi_limited_weights at that faceFlux;  w = fma(lim, cdw, (1.0 - lim)*(fl >= 0 ? 1.0 : 0.0))
 *     v_dir = fma(w, vP - vN, vN)                               (the rule of mi_face_interpolate; rhoU per component with one w)
 *   then, every operator a field operator of the reference and rounded on its own, dir = pos, neg:
 *     U_dir,k = rhoU_dir,k/rho_dir                              (:107-108, three divisions, no reciprocal)
 *     p_dir = rho_dir*rPsi_dir                                  (:110-111)
 *     phiv_dir = fma(U_z, Sf_z, fma(U_x, Sf_x, U_y*Sf_y))       (:113-114, the dot product of DESIGN 3.5a)
 *     cSf_dir = c_dir*magSf                                     (:117-126)
 *     ap = max(max(phiv_pos + cSf_pos, phiv_neg + cSf_neg), 0.0);  am = min(min(phiv_pos - cSf_pos, phiv_neg - cSf_neg), 0.0)
 *                                                               (:128-137; max(a, b) = (a > b) ? a : b, so max(-0.0, 0.0) = +0.0)
 *     a_pos = ap/(ap - am);  amaxSf = max(|am|, |ap|);  aSf = am*a_pos                      (:139-143)
 *     Tadmor: aSf = -0.5*amaxSf;  a_pos = 0.5                                               (:145-149)
 *     a_neg = 1.0 - a_pos;  phiv_pos = phiv_pos*a_pos;  phiv_neg = phiv_neg*a_neg           (:151-154)
 *     aphiv_pos = phiv_pos - aSf;  aphiv_neg = phiv_neg + aSf;  amaxSf = max(|aphiv_pos|, |aphiv_neg|)   (:156-161, the amaxSf written)
 *     phi = aphiv_pos*rho_pos + aphiv_neg*rho_neg                                           (:171, two products and a sum)
 *     phiUp_k = (aphiv_pos*rhoU_pos,k + aphiv_neg*rhoU_neg,k) + (a_pos*p_pos + a_neg*p_neg)*Sf_k         (:173-177)
 *     phiEp = ((aphiv_pos*(rho_pos*(e_pos + 0.5*magSqr(U_pos)) + p_pos) + aphiv_neg*(rho_neg*(e_neg + 0.5*magSqr(U_neg)) + p_neg))
 *              + aSf*p_pos) - aSf*p_neg                                                     (:179-185, left to right as written)
 *     magSqr(U) = fma(U_z, U_z, fma(U_x, U_x, U_y*U_y)): magSqr contracts as the dot product does -- an ASSUMPTION
 *     a_pos_out, au_out (all four or none): a_pos and aU_k = a_pos*U_pos,k + a_neg*U_neg,k (what sigmaDotU, :216-224, reads)
 *   ap - am == 0 (it needs c == 0) has no special case: the reference's NaN comes out.  One launch, one thread per face, no atomics, the
 *   same bits on every run; under the context's launch-grid cap (MI_FACE_GRID).
 * mi_patch_central_flux: one patch.  patch_weights NULL (any patch that is not coupled): `values` holds the seven BOUNDARY VALUE arrays
 *   (rho, rhoU[3], rPsi, e, c per patch face; no gradient is read), which are the face values of both directions
 *   (surfaceInterpolationScheme.C:261-264); the algebra above runs operation for operation, nothing simplified.  patch_weights given (a
 *   COUPLED patch): `values` the cell arrays (read through the patch's faceCells), `nbr` their patchNeighbourFields, d = patch_delta, the
 *   limiter as mi_patch_limited_weights', v_dir = w*vP + (1.0 - w)*vNbr with every operator rounded (surfaceInterpolationScheme.C:361-366).
 * mi_central_sound_speed (:84, :116): rPsi = 1.0/psi;  c = sqrt((Cp/Cv)*rPsi) in that order, IEEE / and sqrt.
 * mi_central_courant (compressibleCourantNo.H:35-47): max over the internal AND the boundary faces of (deltaCoeffs*amaxSf)/magSf
 *   (max(GeometricField) includes the boundary, GeometricFieldFunctions.C:478-506) and sum over the INTERNAL faces of deltaCoeffs*amaxSf
 *   (sum(GeometricField) does not, :511-538), to the host; the caller multiplies by deltaT and divides by its own sum(magSf).  The product
 *   is formed on load in the reduction trees of mi_sum and mi_min_max: the sum is mi_sum's over the stored product bit for bit, the max
 *   mi_min_max's.  No internal faces: 0 and 0, no launch.  During a PCG session: MI_ERR_STATE.
 * Refused (MI_ERR_ARG, nothing launched, nothing written): an invalid mi_central_scheme; a missing array; internal-face arrays not 16-byte
 *   aligned, cell and patch arrays not 8-byte aligned; an output that aliases an input or another output; a_pos_out / au_out given in
 *   part; a scalar reconstruct(U) without lim_u and its gradient.  A mesh without internal faces, a patch without faces: MI_OK, no launch.
 * Out of scope: the viscous branch and sigmaDotU (apart from aU), rhoCentralDyMFoam's mesh-flux terms, the slip and jump boundary
 *   conditions of rhoCentralFoam/BCs, rotated coupled patches. */
enum { MI_CENTRAL_KURGANOV = 0, MI_CENTRAL_TADMOR = 1 };
typedef struct mi_central_scheme {
    int32_t flux_scheme, reserved;            /* MI_CENTRAL_* */
    mi_limiter rho, U, T;                     /* reconstruct(rho), reconstruct(U), reconstruct(T) */
} mi_central_scheme;
typedef struct mi_central_cells {             /* one side's fields: cell arrays, patchNeighbourFields, or a plain patch's boundary values */
    const double *rho_dev, *rhou_dev[3], *rpsi_dev, *e_dev, *c_dev;
    const double *grad_rho_dev[3], *grad_rhou_dev[9], *grad_rpsi_dev[3], *grad_e_dev[3], *grad_c_dev[3];   /* grad_rhou[3*j + k] = d(rhoU_j)/dx_k: a V reconstruct(U) only */
    const double *lim_u_dev, *grad_lim_u_dev[3];   /* a scalar reconstruct(U) only: magSqr(rhoU) and its gradient */
} mi_central_cells;
typedef struct mi_central_out {
    double *phi_out_dev, *phiup_out_dev[3], *phiep_out_dev, *amaxsf_out_dev;
    double *a_pos_out_dev, *au_out_dev[3];    /* all four or all NULL */
} mi_central_out;
int mi_central_scheme_parse(const char *flux_scheme, const char *reconstruct_rho, const char *reconstruct_U, const char *reconstruct_T,
                            mi_central_scheme *out);
int mi_central_flux(mi_addr_t addr, const mi_central_scheme *scheme, const double *cd_weights_dev, const double *const *sf_dev,
                    const double *mag_sf_dev, const mi_central_cells *cells, const double *const *c_dev, const mi_central_out *out);
int mi_patch_central_flux(mi_patch_t patch, const mi_central_scheme *scheme, const double *patch_weights_dev_or_null,
                          const double *const *patch_sf_dev, const double *patch_mag_sf_dev, const mi_central_cells *values,
                          const mi_central_cells *nbr_or_null, const double *const *patch_delta_dev_or_null, const mi_central_out *out);
int mi_central_sound_speed(mi_ctx_t ctx, int64_t n, const double *cp_dev, const double *cv_dev, const double *psi_dev,
                           double *rpsi_out_dev, double *c_out_dev);
int mi_central_courant(mi_addr_t addr, const double *delta_coeffs_dev, const double *mag_sf_dev, const double *amaxsf_dev,
                       int64_t n_boundary, const double *b_delta_coeffs_dev, const double *b_mag_sf_dev, const double *b_amaxsf_dev,
                       double *max_out_host, double *sum_out_host);
/* ---- the LES models Smagorinsky, oneEqEddy and dynOneEqEddy with cubeRootVolDelta and the simpleFilter
 *      (turbulenceModels/incompressible/LES/Smagorinsky/Smagorinsky.C:45-49, Smagorinsky.H:117-120; oneEqEddy/oneEqEddy.C:46-50, :100-122,
 *      oneEqEddy.H:132; dynOneEqEddy/dynOneEqEddy.C:45-100, :134-137, :145-172; GenEddyVisc/GenEddyVisc.C:61;
 *      turbulenceModels/LES/LESfilters/simpleFilter/simpleFilter.C:64-125; LES/LESdeltas/cubeRootVolDelta/cubeRootVolDelta.C:42-76;
 *      LES/LESdeltas/LESdelta/LESdelta.C:53) ----
 * One correct() of dynOneEqEddy calls an LESfilter thirteen times inside about thirty field operators, roughly a hundred field passes; here it
 * is four cell passes and five row passes, beside the k equation's assembly, relaxation, solve and mi_bound.  The rules of the kEpsilon block
 * hold: fp64 values, int32 labels, every operator rounded on its own except the fma written below, IEEE / and sqrt, max(a, b) = (a > b) ? a : b,
 * mag = fabs, the face order of mi_fvc_average.  A symmetric tensor is six arrays in the order xx, xy, xz, yy, yz, zz; grad_dev is
 * mi_ke_production's layout.  SMALL = 1e-15, VSMALL = 1e-300.  Field operators of the reference are separate passes over stored fields, so
 * nothing is contracted ACROSS them (fSqrU - sqr(fU) is a rounded product, then a subtraction); inside one primitive operator:
 *   dev(st)   (SymmTensorI.H:326-329): t = (1.0/3.0)*((xx + yy) + zz); xx - t, yy - t, zz - t: no fma (the product has three uses)
 *   a && b    (SymmTensorI.H:233-241): s = fma(a.xx, b.xx, (2*a.xy)*b.xy); s = fma(2*a.xz, b.xz, s); s = fma(a.yy, b.yy, s);
 *             s = fma(2*a.yz, b.yz, s); s = fma(a.zz, b.zz, s)
 *   magSqr(v) (VectorSpaceI.H:336-344): fma(v.z, v.z, fma(v.x, v.x, v.y*v.y))
 *   magSqr(st): the chain stated for mi_ke_production
 *   read from LLVM's contraction of these expressions (an ASSUMPTION for the device compiler).
 * mi_les_simple_filter (simpleFilter.C:64-125) on a mi_average_t: out_k = surfaceSum(magSf*interpolate(vf_k))/surfaceSum(magSf) for
 *   k < n_cmpt, 1 <= n_cmpt <= 9 (nine: a volTensorField), in ONE row pass that writes no face field.  Per face, for component k:
 *     i = fma(lambda, P_k - N_k, N_k);  p = magSf*i (rounded);  s_k = s_k + p
 *   own faces ascending, neighbour-side faces in losort order, then the boundary faces patch by patch with p = b_magSf*b_face_k;
 *   out_k[c] = s_k/sum[c]: ONE DIVISION PER COMPONENT -- VectorSpace's operator/(vs, scalar) (VectorSpaceI.H:621-630) applies divideOp3,
 *   `x / y` (ops.H:208), to every component; it does not multiply by a reciprocal.  A cell without faces gives 0/0.  b_face_dev[k]: the
 *   patch-ordered boundary face values of the UNFILTERED field, the caller's: its boundary values on a non-coupled patch,
 *   w*P + (1 - w)*Nbr on a coupled one.  The filtered field's own boundary values are zero-gradient (fvcSurfaceIntegrate.C:285):
 *   mi_patch_internal_field.  Only the first n_cmpt pointers of vf_dev, b_face_dev and out_dev are read.
 * mi_les_delta_cube_root_vol (cubeRootVolDelta.C:48, :68): thickness_or_0 == 0: out = deltaCoeff*pow(V, 1.0/3.0), the device library's pow,
 *   not cbrt; thickness_or_0 > 0 (a 2-D case): out = deltaCoeff*sqrt(V/thickness).  pow_out_dev_or_null receives the root (for tests).
 *   delta's BOUNDARY values stay the constructor's SMALL (LESdelta.C:53: calculated patches, calcDelta sets the internal field only): the
 *   boundary array is the caller's, filled with SMALL.
 * mi_les_coeffs_init (host only): ck and ce, the reference's defaults 0.094 (Smagorinsky.C:72, oneEqEddy.C:86) and 1.048 (GenEddyVisc.C:61);
 *   a non-finite or non-positive member is refused, here and by every entry that takes a mi_les_coeffs.
 * mi_les_smagorinsky (Smagorinsky.H:119, Smagorinsky.C:47): k = (((2.0*ck)/ce)*(delta*delta))*magSqr(dev(symm(gradU))), (2.0*ck)/ce formed on
 *   the host; nuSgs = (ck*delta)*sqrt(k).
 * mi_les_k_terms (oneEqEddy.C:104-113, dynOneEqEddy.C:154-163, oneEqEddy.H:132): G = (2.0*nuSgs)*magSqr(symm(gradU)) through the device
 *   function of mi_ke_production, hence with its bits for nut = nuSgs; sp = (ce*sqrt(k))/delta with ce the number, or per cell when
 *   ce_dev_or_null is given (the dynamic model); dk = nuSgs + nu, nu a cell array or nu_value.  G and sp are mi_fvm_assemble's su_dev and sp_dev.
 * mi_les_nusgs (oneEqEddy.C:48, dynOneEqEddy.C:51): out = (ck*sqrt(k))*delta, ck the number or per cell.
 * The dynamic procedure (dynOneEqEddy.C:56-100, :136, :151-152).  Every cell pass is a per-element map without neighbour access: run over
 *   the patch-ordered boundary arrays it gives the boundary values of its outputs on non-coupled patches, as the reference's field algebra
 *   forms them.  With delta_b = SMALL, MM_b all but vanishes and ce_den_b is enormous: the reference's result, replicated.
 *   mi_les_dyn_moments: sqr(U) (SymmTensorI.H:546-554), magSqr(U), D = symm(gradU) (0.5*(a + b) off the diagonal), magSqr(D).
 *   level 1 (filter_): U (3), sqr(U) (6), magSqr(U), D (6), magSqr(D): 17 components in two mi_les_simple_filter launches (9 + 8).
 *   mi_les_dyn_level1: KK = 0.5*(fMagSqrU - magSqr(fU)), with clip != 0 then KK = max(KK, SMALL) (correct() :152 clips, the constructor :136
 *     does not); LL = dev(a) with a_ij = fSqrU_ij - fU_i*fU_j; MM = ((-2.0*delta)*sqrt(KK))*fD; ce_num = nuEff*(fMagSqrD - magSqr(fD));
 *     ce_den = pow(KK, 1.5)/(2.0*delta), the device library's pow evaluated once; pow_out_dev_or_null receives it (for tests).
 *   level 2 (simpleFilter_): LL, MM, ce_num, ce_den: 14 components in two launches.
 *   mi_les_dyn_level2: lm = 0.5*(fLL && fMM); mmmm = magSqr(fMM).   level 3: lm and mmmm, one launch of 2 components.
 *   mi_les_dyn_coeffs (:72-99): c = f_lm/(f_mmmm + VSMALL), ck = 0.5*(mag(c) + c); e = f_ce_num/f_ce_den, ce = 0.5*(mag(e) + e).
 * The cell passes take two cells per thread with 16-byte accesses when every array is 16-byte aligned, one by one otherwise, under the
 *   context's launch-grid cap (MI_FACE_GRID).
 * Refused (MI_ERR_ARG, nothing launched, nothing written): n_cmpt outside 1..9; a missing array; an output that aliases an input or another
 *   output (reported before alignment, as mi_fvc_average does); an array not aligned for a double; NULL boundary arrays while the boundary
 *   has faces; a handle of another addressing; a coefficient that is not finite or not above zero.  Zero cells: MI_OK.
 * Out of scope: laplaceFilter and anisotropicFilter; vanDriestDelta, smoothDelta, maxDeltaxyz and PrandtlDelta (they need the wall distance
 *   or face geometry); the homogeneous dynamic models (their average() fixes a reduction order); the Spalart-Allmaras DES family (the block below); the nuSgs
 *   wall functions; compressible LES; a pisoFoam application; moving meshes. */
typedef struct mi_les_coeffs {
    double ck, ce;
} mi_les_coeffs;
int mi_les_coeffs_init(double ck, double ce, mi_les_coeffs *out);
int mi_les_simple_filter(mi_average_t average, int n_cmpt, const double *lambda_dev, const double *mag_sf_dev, const double *b_mag_sf_dev,
                         const double *const *vf_dev, const double *const *b_face_dev, double *const *out_dev);
int mi_les_delta_cube_root_vol(mi_ctx_t ctx, int64_t n, double delta_coeff, double thickness_or_0, const double *v_dev, double *out_dev,
                               double *pow_out_dev_or_null);
int mi_les_smagorinsky(mi_ctx_t ctx, int64_t n, const mi_les_coeffs *coeffs, const double *delta_dev, const double *const *grad_dev,
                       double *k_out_dev_or_null, double *nusgs_out_dev);
int mi_les_k_terms(mi_ctx_t ctx, int64_t n, double ce, const double *ce_dev_or_null, const double *nusgs_dev, const double *const *grad_dev,
                   const double *k_dev, const double *delta_dev, const double *nu_dev_or_null, double nu_value, double *g_out_dev,
                   double *sp_out_dev, double *dk_out_dev);
int mi_les_nusgs(mi_ctx_t ctx, int64_t n, double ck, const double *ck_dev_or_null, const double *k_dev, const double *delta_dev, double *out_dev);
int mi_les_dyn_moments(mi_ctx_t ctx, int64_t n, const double *const *u_dev, const double *const *grad_dev, double *const *sqr_u_out_dev,
                       double *magsqr_u_out_dev, double *const *d_out_dev, double *magsqr_d_out_dev);
int mi_les_dyn_level1(mi_ctx_t ctx, int64_t n, int clip, const double *delta_dev, const double *nueff_dev, const double *const *f_u_dev,
                      const double *const *f_sqr_u_dev, const double *f_magsqr_u_dev, const double *const *f_d_dev,
                      const double *f_magsqr_d_dev, double *kk_out_dev, double *const *ll_out_dev, double *const *mm_out_dev,
                      double *ce_num_out_dev, double *ce_den_out_dev, double *pow_out_dev_or_null);
int mi_les_dyn_level2(mi_ctx_t ctx, int64_t n, const double *const *f_ll_dev, const double *const *f_mm_dev, double *lm_out_dev,
                      double *mmmm_out_dev);
int mi_les_dyn_coeffs(mi_ctx_t ctx, int64_t n, const double *f_lm_dev, const double *f_mmmm_dev, const double *f_ce_num_dev,
                      const double *f_ce_den_dev, double *ck_out_dev, double *ce_out_dev);
/* ---- the Spalart-Allmaras model: RAS, DES, DDES, IDDES and the nutUSpalding wall function
 *      (turbulenceModels/incompressible/RAS/SpalartAllmaras/SpalartAllmaras.C:45-137, :190, :269-275, :437-464;
 *      LES/SpalartAllmaras/SpalartAllmaras.C:45-172, :260, :331-357; LES/SpalartAllmarasDDES/SpalartAllmarasDDES.C:45-93;
 *      LES/SpalartAllmarasIDDES/SpalartAllmarasIDDES.C:45-140; RAS/derivedFvPatchFields/wallFunctions/nutWallFunctions/
 *      nutUSpaldingWallFunction/nutUSpaldingWallFunctionFvPatchScalarField.C:39-110; fvMatrix.C:2208-2216, :2731-2756, :2773-2800; fvmSup.C:100-131;
 *      primitives/Scalar/Scalar.H:183-204) ----
 * correct() of the RAS class is about 30 one-operator field passes between the gradients and the matrix, of IDDES well over 80; here it is ONE
 * cell pass, mi_sa_terms, beside the gradients, mi_fvm_assemble, mi_relax, the solve, mi_bound and mi_sa_nut.  The rules of the kEpsilon and
 * LES blocks hold: fp64 values, int32 labels, every field operator rounded on its own except the fma written below, IEEE / and sqrt,
 * max(a, b) = (a > b) ? a : b, min(a, b) = (a < b) ? a : b, pos(x) = x >= 0, neg(x) = x < 0, pow3(s) = s*sqr(s), pow6(s) = pow3(sqr(s))
 * (Scalar.H:183-204), SMALL = 1e-15, ROOTVSMALL = 1e-150.  grad_dev is mi_ke_production's layout, g[3*j + k] = d(U_j)/dx_k.  y (wallDist),
 * delta (LESdelta / IDDESDelta) and hmax (maxDeltaxyz) are the CALLER's cell arrays.  pow, tanh and exp are the device library's and NOT the
 * reference's bits: each is evaluated once per cell and can be returned, and everything formed from them is exact given them.  A per-element
 * map has no neighbour access: run over the patch-ordered boundary arrays it gives the boundary values (the rule of the LES block).
 *   magSqr(v)  of grad(nuTilda): fma(v.z, v.z, fma(v.x, v.x, v.y*v.y))                                          (stated in the LES block)
 *   mag(symm(gradU)): sqrt of the chain stated for mi_ke_production
 *   mag(skew(gradU)) (TensorI.H:511-519, VectorSpaceI.H:336-355): magSqr of the nine components t0..t8 is s = fma(t0, t0, t1*t1), then
 *     s = fma(tk, tk, s) for k = 2..8; skew's diagonal is 0.0, so with xy = 0.5*(g1 - g3), xz = 0.5*(g2 - g6), yx = 0.5*(g3 - g1),
 *     yz = 0.5*(g5 - g7), zx = 0.5*(g6 - g2), zy = 0.5*(g7 - g5):  s = xy*xy, then fma(xz, xz, s), fma(yx, yx, s), fma(yz, yz, s),
 *     fma(zx, zx, s), fma(zy, zy, s); mag = sqrt(s)                                             (an ASSUMPTION)
 * mi_sa_coeffs_init (host only, no GPU): model_or_null = {sigmaNut, kappa, Cb1, Cb2, Cw2, Cw3, Cv1, Cv2, CDES, ck, fwStar, cl, ct}, NULL for
 *   the reference's defaults 0.66666, 0.41, 0.1355, 0.622, 0.3, 2.0, 7.1, 5.0, 0.65, 0.07, 0.424, 3.55, 1.63; wall_or_null = {kappa, E} of the
 *   wall function, NULL for 0.41, 9.8.  The products of dimensionedScalars are formed once, in the reference's operand order:
 *   Cw1 = Cb1/sqr(kappa) + (1.0 + Cb2)/sigmaNut, Cb2BySigmaNut = Cb2/sigmaNut, Cv1_3 = pow3(Cv1), Cw3_6 = pow6(Cw3), onePlusCw3_6 = 1 + Cw3_6,
 *   invCv2 = 1/Cv2, ct2 = sqr(ct), cl2 = sqr(cl), psiDen = (Cw1*sqr(kappa))*fwStar, psiCoeff = Cb1/psiDen, invE = 1/E, sqrt2 = sqrt(2.0).
 *   Every member must be finite and above zero, here and in every entry that takes a mi_sa_coeffs.
 * mi_sa_terms: kind = MI_SA_RAS | MI_SA_DES | MI_SA_DDES | MI_SA_IDDES, ashford != 0: ashfordCorrection.  With nt = nuTilda:
 *     chi = nt/nu;  chi3 = pow3(chi);  fv1 = chi3/(chi3 + Cv1_3)                                                  (RAS :51-55, LES :54-58)
 *     S = sqrt2*mag(skew(gradU)); for MI_SA_DDES sqrt2*mag(symm(gradU)) -- SpalartAllmarasDDES::S overrides the virtual (DDES.C:78-81),
 *       SpalartAllmarasIDDES does not
 *     Ashford, RAS (:66, :83-89):  fv2 = 1.0/pow3(1 + chi/Cv2);          c = invCv2*chi
 *     Ashford, LES (:65, :79-86):  fv2 = 1/pow3(1 + nt/(Cv2*nu));        c = chi/Cv2
 *              both:               fv3 = (((1 + chi*fv1)*invCv2)*(3*(1 + c) + sqr(c)))/pow3(1 + c)
 *     without Ashford:             fv2 = 1.0 - chi/(1.0 + chi*fv1);      fv3 = 1
 *     dTilda   RAS: y.   DES (:169-172): min(CDES*delta, y).
 *              rd(visc) = min(visc/(max(S, SMALL)*sqr(kappa*y) + ROOTVSMALL), 10)                               (DDES :45-69, IDDES :73-97)
 *              DDES (:72-93): fd = 1 - tanh(pow3(8*rd(nuSgs + nu)));  dTilda = max(y - fd*max(y - CDES*delta, 0), SMALL)
 *              IDDES (:45-140): alpha = max(0.25 - y/hmax, -5);  e = exp(sqr(alpha));  p1 = pow(e, -11.09);  p2 = pow(e, -9.0)
 *                fHill = 2*(pos(alpha)*p1 + neg(alpha)*p2);  fStep = min(2*p2, 1);  fd as DDES;  fHyb = max(1 - fd, fStep)
 *                ft = tanh(pow3(ct2*rd(nuSgs)));  fl = tanh(pow(cl2*rd(nu), 10));  fAmp = 1 - max(ft, fl)
 *                fRestore = max(fHill - 1, 0)*fAmp;  Psi = sqrt(min(100, (1 - psiCoeff*fv2)/max(SMALL, fv1)))
 *                dTilda = max(SMALL, (fHyb*(1 + fRestore*Psi))*y + (((1 - fHyb)*CDES)*Psi)*delta)
 *     STilda   RAS (:440-444): (fv3*sqrt2)*mag(skew(gradU)) + (fv2*nt)/sqr(kappa*y)    -- sqrt(2.0) meets fv3 BEFORE the magnitude
 *              LES (:123):     fv3*S + (fv2*nt)/sqr(kappa*dTilda)
 *     r        RAS (:116-131): min(nt/(max(STilda, SMALL)*sqr(kappa*y)), 10)           -- no ROOTVSMALL
 *              LES (:127-153): min(nt/(max(STilda, SMALL)*sqr(kappa*dTilda) + ROOTVSMALL), 10)
 *     g = r + Cw2*(pow6(r) - r);  fw = g*pow(onePlusCw3_6/(pow6(g) + Cw3_6), 1.0/6.0)                              (RAS :134-136, LES :163-165)
 *     su_grad = Cb2BySigmaNut*magSqr(grad(nt));  su_prod = (Cb1*STilda)*nt;  sp = ((Cw1*fw)*nt)/sqr(dTilda);  dnu = (nt + nu)/sigmaNut
 *   nu a cell array, or nu_value when nu_dev_or_null is NULL.  delta is read by the DES kinds, nuSgs by DDES and IDDES, hmax by IDDES; an
 *   array a kind does not read may be NULL.  Optional outputs (NULL: not written): S, dTilda, STilda and pow of fw for every kind; tanh of fd
 *   for DDES and IDDES; e, p1, p2, ft, pow(., 10) and fl for IDDES.  One that the kind does not form is refused.
 *   The equation (RAS :446-455, LES :335-349): ddt + div - laplacian - su_grad == su_prod - fvm::Sp(sp, nt).  operator-(tmp<fvMatrix>,
 *   tmp<volScalarField>) adds V*su_grad to the left side's source (fvMatrix.C:2731-2756: `tC().source() += V*su`);
 *   operator-(tmp<volScalarField>, fvMatrix) negates the Sp matrix and subtracts V*su_prod from ITS source (:2773-2800); operator== subtracts that
 *   matrix: diag = diagL + V*sp, source = (sourceL + V*su_grad) + V*su_prod -- two additions in this order, not V*(su_grad + su_prod).  That
 *   is mi_fvm_assemble with sp_sign > 0, n_su = 2, su = {su_grad, su_prod} and both su_sign < 0; no entry of its own.
 * mi_sa_nut: recompute_fv1 == 0 (RAS :463): nut = fv1*nt with fv1_dev_or_null the array mi_sa_terms wrote BEFORE the solve;
 *   recompute_fv1 != 0 (updateSubGridScaleFields, LES :45-49, and the constructor): fv1 recomputed from nt and nu, optionally returned.
 * mi_sa_nut_spalding_wall (nutUSpalding :93-110 with calcUTau's functor :39-89): every wall face of ALL wall patches in ONE launch on a
 *   mi_ke_t, one thread per face, no atomics.  Per face with cell c (mag as in mi_ke_wall_cells):
 *     magUp = mag(U[c] - Uw);  magGradU = mag(dc*(Uw - U[c]));  ut = sqrt((nutw + nuw)*magGradU)
 *     ut <= ROOTVSMALL: uTau = 0.  Otherwise at most ten times:
 *       kUu = min((kappa*magUp)/ut, 50);  e = exp(kUu);  fkUu = fma(-kUu, fma(kUu, 0.5, 1.0), e - 1)
 *       f = fma(invE, fma(-(1.0/6.0)*kUu, sqr(kUu), fkUu), magUp/ut - (ut*y)/nuw)
 *       df = (magUp/sqr(ut) + y/nuw) + ((invE*kUu)*fkUu)/ut;  new = ut + f/df;  err = mag((ut - new)/ut);  ut = new
 *     while ut > ROOTVSMALL && err > 0.01 && ++iter < 10;  uTau = max(0.0, ut)     (the contraction: an ASSUMPTION)
 *     nutw = max(0, sqr(uTau)/(magGradU + ROOTVSMALL) - nuw)
 *   b_nutw_inout_dev holds the patch-ordered boundary values of nut: a wall face reads its own value and writes the new one, other faces are
 *   untouched.  b_exp_out_dev_or_null (10 per BOUNDARY face, [10*face + step]) receives e of every step taken, b_iter_out_dev_or_null (int32
 *   per boundary face) the number of steps; faces that are not on a wall and steps not taken are not written.
 * Refused (MI_ERR_ARG, nothing launched, nothing written): as in the LES block -- missing arrays (delta for the DES kinds, nuSgs for DDES and
 *   IDDES, hmax for IDDES), an output that aliases an input or another output, an array not aligned for a double, a handle of another
 *   addressing, coefficients that are not finite or not above zero, a nu_value that is not, an unknown kind.  Zero cells, zero wall faces: MI_OK.
 * Out of scope: wallDist / meshWave, maxDeltaxyz and IDDESDelta (y, hmax and delta are the caller's arrays); nuSgsUSpaldingWallFunction and the
 *   other wall functions; k(), epsilon(), B(), LESRegion() beyond the dTilda output; the compressible forms; moving meshes; a simpleFoam /
 *   pisoFoam application; the wiring into tools/workloads.py. */
#define MI_SA_RAS 0
#define MI_SA_DES 1
#define MI_SA_DDES 2
#define MI_SA_IDDES 3
typedef struct mi_sa_coeffs {
    double sigmaNut, kappa, Cb1, Cb2, Cw2, Cw3, Cv1, Cv2, CDES, ck, fwStar, cl, ct;
    double wallKappa, E;                      /* the wall function's */
    double Cw1, Cb2BySigmaNut, Cv1_3, Cw3_6, onePlusCw3_6, invCv2, ct2, cl2, psiDen, psiCoeff, invE, sqrt2;   /* derived: mi_sa_coeffs_init */
} mi_sa_coeffs;
typedef struct mi_sa_cells {
    const double *nutilda_dev;
    const double *grad_dev[9];
    const double *grad_nutilda_dev[3];
    const double *y_dev;
    const double *nu_dev_or_null;
    double nu_value;
    const double *delta_dev, *nusgs_dev, *hmax_dev;
    double *su_grad_out_dev, *su_prod_out_dev, *sp_out_dev, *dnu_out_dev, *fv1_out_dev;
    double *s_out_dev_or_null, *dtilda_out_dev_or_null, *stilda_out_dev_or_null, *pow_fw_out_dev_or_null;
    double *tanh_fd_out_dev_or_null;
    double *exp_out_dev_or_null, *pow_hill_pos_out_dev_or_null, *pow_hill_neg_out_dev_or_null, *tanh_ft_out_dev_or_null, *pow_fl_out_dev_or_null,
           *tanh_fl_out_dev_or_null;
} mi_sa_cells;
typedef struct mi_sa_wall {
    const double *u_dev[3];
    const double *b_uw_dev[3];                /* the boundary face values of U */
    const double *b_delta_coeffs_dev, *b_y_dev, *b_nuw_dev;
    double *b_nutw_inout_dev;
    double *b_exp_out_dev_or_null;
    int32_t *b_iter_out_dev_or_null;
} mi_sa_wall;
int mi_sa_coeffs_init(const double *model_or_null, const double *wall_or_null, mi_sa_coeffs *out);
int mi_sa_terms(mi_ctx_t ctx, int64_t n, const mi_sa_coeffs *coeffs, int kind, int ashford, const mi_sa_cells *arrays);
int mi_sa_nut(mi_ctx_t ctx, int64_t n, const mi_sa_coeffs *coeffs, int recompute_fv1, const double *nutilda_dev, const double *fv1_dev_or_null,
              const double *nu_dev_or_null, double nu_value, double *nut_out_dev, double *fv1_out_dev_or_null);
int mi_sa_nut_spalding_wall(mi_ke_t ke, const mi_sa_coeffs *coeffs, const mi_sa_wall *arrays);
/* ---- the compressible operators of rhoPimpleFoam (BASELINE config 5; round 5) ----
 * mi_fvm_ddt_euler_rho: fvm::ddt(rho, vf) with a density FIELD -- EulerDdtScheme<Type>::fvmDdt(const volScalarField& rho, vf),
 *   src/finiteVolume/finiteVolume/ddtSchemes/EulerDdtScheme/EulerDdtScheme.C:403-440:
 *     diag = rDeltaT*rho*V, source = rDeltaT*rho.oldTime()*vf.oldTime()*V   (rhoPimpleFoam/UEqn.H:5, EEqn.H:6; with psi in rho's
 *   place fvm::ddt(psi, p), pEqn.H:38,62).
 * mi_fvm_su / mi_fvm_sp / mi_fvm_susp: src/finiteVolume/finiteVolume/fvm/fvmSup.C:34-54 (source -= V*su), :100-170 (diag += V*sp;
 *   sp_dev NULL => the dimensionedScalar form with sp_value), :190-214 (diag += V*max(susp,0); source -= V*min(susp,0)*vf) -- in
 *   place on the matrix's diagonal / source (fvOptions(rho, U), the explicit terms of EEqn.H).
 * mi_flux_div: phi = Sf & linear-interpolate([cell_scale *] V) [+ add_a [* add_b]] on the internal faces AND
 *   div = fvc::surfaceIntegrate(phi) [/ vol] in one call -- pEqn.H:49-71's
 *   phiHbyA = (fvc::interpolate(rho*HbyA) & mesh.Sf()) + rhorAUf*fvc::ddtCorr(rho, U, phi) followed by fvc::div(phiHbyA)
 *   (finiteVolume/fvc/fvcSurfaceIntegrate.C:40-96), which the reference computes with seven field passes: here one face pass
 *   (rho*HbyA, the three interpolates, the dot product, the product and the sum at once) + the row sum.  lambda = the
 *   interpolation weights (surfaceInterpolationScheme.C:275-280); boundary faces: mi_patch_add on div as the reference adds them.
 * mi_ddt_phi_corr: fvc::ddtCorr(rho, U, phi) on the internal faces, EulerDdtScheme<Type>::fvcDdtPhiCorr(rho, U, phi)
 *   (EulerDdtScheme.C:663-720, first branch; rho_old NULL: fvcDdtPhiCorr(U, phi) :523-551) with ddtScheme<Type>::fvcDdtPhiCoeff
 *   (ddtSchemes/ddtScheme/ddtScheme.C:139-174) in one face pass:
 *     phiCorr = phi0 - (Sf & interpolate(rho0*U0)); out = (1 - min(|phiCorr|/(|phi0| + SMALL), 1))*rDeltaT*phiCorr.          */
int mi_fvm_ddt_euler_rho(mi_ctx_t ctx, int64_t n, double r_delta_t, const double *rho_dev, const double *rho_old_dev,
                         const double *vol_dev, const double *psi_old_dev, double *diag_out_dev, double *source_out_dev);
int mi_fvm_su(mi_ctx_t ctx, int64_t n, const double *vol_dev, const double *su_dev, double *source_inout_dev);
int mi_fvm_sp(mi_ctx_t ctx, int64_t n, const double *vol_dev, const double *sp_dev_or_null, double sp_value, double *diag_inout_dev);
int mi_fvm_susp(mi_ctx_t ctx, int64_t n, const double *vol_dev, const double *susp_dev, const double *vf_dev,
                double *diag_inout_dev, double *source_inout_dev);
int mi_flux_div(mi_addr_t addr, const double *lambda_dev, const double *sfx_dev, const double *sfy_dev, const double *sfz_dev,
                const double *vx_dev, const double *vy_dev, const double *vz_dev, const double *cell_scale_dev_or_null,
                const double *add_a_dev_or_null, const double *add_b_dev_or_null, double *phi_out_dev,
                const double *vol_dev_or_null, double *div_out_dev);
int mi_ddt_phi_corr(mi_addr_t addr, double r_delta_t, const double *lambda_dev, const double *sfx_dev, const double *sfy_dev,
                    const double *sfz_dev, const double *ux_old_dev, const double *uy_old_dev, const double *uz_old_dev,
                    const double *rho_old_dev_or_null, const double *phi_old_dev, double *out_dev);
/* ---- fused matrix assembly (round 6) ----
 * mi_fvm_assemble: the matrix of   [fvm::ddt(rho, vf)] + [fvm::div(flux, vf)] - [fvm::laplacian(gamma, vf)] [+- fvm::Sp(sp, vf)] [+- su ...]
 * written ONCE by one row pass -- the expression every transport equation of simpleFoam / pisoFoam / rhoPimpleFoam has
 * (UEqn.H, EEqn.H, pEqn.H) and that the reference evaluates scheme by scheme (gaussConvectionScheme.C:74-115, gaussLaplacianScheme.C:44-88,
 * EulerDdtScheme.C:371-440, fvmSup.C:34-214) and then combines array by array with fvMatrix::operator+ / - / == (fvMatrix.C:1693-2030 ->
 * lduMatrix::operator+= / -=, lduMatrixOperations.C:235-396).  The outputs equal that sequence BIT FOR BIT, because every intermediate is
 * rounded where the sequence rounds it:
 *   per face    lB = -w*flux, uB = lB + flux (w = div_weights, or pos(flux) when div_weights_dev is NULL: upwind);  uL = deltaCoeffs*gammaMagSf
 *               lower = lB - uL, upper = uB - uL   (a term that is absent drops out of the expression; no convection: upper = -uL, the
 *               matrix stays symmetric and lower_out_dev may be NULL)
 *   per cell    sumB = negSumDiag of (lB, uB), sumL = negSumDiag of (uL, uL)   (lduMatrixOperations.C:61-83: own faces ascending, then losort order)
 *               diag = (((rDeltaT*rho)*V + sumB) - sumL) [+- V*sp]
 *               source[r] = ((rDeltaT*rho_old)*psi_old[r])*V, then  -= V*su[k][r] (su_sign[k] > 0: the term stands on the left, `+ su`)
 *               or += V*su[k][r] (su_sign[k] < 0: `== su`), k ascending      (fvMatrix.C:1850-1905 operator+/-(fvMatrix, volField), :1741 operator==)
 * rho_dev NULL: the constant rho_value (fvm::ddt(vf): 1).  su_dev holds n_su * n_rhs device pointers, su_dev[k * n_rhs + r]; su_sign
 * n_su host doubles.  n_rhs <= 4 right-hand sides share the coefficients (the components of a vector equation, fvMatrixSolve.C:103-225),
 * n_su <= 4.  sum_mag_off_diag_out_dev (may be NULL): lduMatrix::sumMagOffDiag of the FINAL coefficients from the same pass -- what
 * fvMatrix::relax needs (mi_relax_multi takes it).  Boundary coefficients stay with the caller (mi_patch_add), as in the reference.
 * Coefficient outputs must not alias inputs (faces cut by a block boundary are recomputed from the inputs).                          */
typedef struct mi_fvm_terms {
    int32_t ddt;                                   /* != 0: Euler time derivative present */
    double r_delta_t, rho_value;
    const double *rho_dev, *rho_old_dev;           /* both NULL (constant rho_value) or both given */
    const double *vol_dev;                         /* needed with ddt, sp or su */
    const double *div_flux_dev, *div_weights_dev;  /* flux NULL: no convection term */
    const double *lap_delta_coeffs_dev, *lap_gamma_magsf_dev;   /* delta NULL: no diffusion term */
    const double *sp_dev; double sp_sign;          /* sp NULL: none; sign > 0: diag += V*sp, < 0: diag -= V*sp */
    int32_t n_rhs; const double *const *psi_old_dev;   /* n_rhs old-time fields (read when ddt != 0) */
    int32_t n_su; const double *const *su_dev; const double *su_sign;
} mi_fvm_terms;
int mi_fvm_assemble(mi_addr_t addr, const mi_fvm_terms *terms, double *lower_out_dev_or_null, double *upper_out_dev, double *diag_out_dev,
                    double *const *source_out_dev, double *sum_mag_off_diag_out_dev_or_null);
/* ---- explicit correction of the corrected convection schemes linearUpwind and LUST ----
 * `Gauss linearUpwind grad(U)` / `Gauss LUST grad(U)`: gaussConvectionScheme<Type>::fvmDiv (src/finiteVolume/finiteVolume/convectionSchemes/
 * gaussConvectionScheme/gaussConvectionScheme.C:109-112) adds   fvm += fvc::surfaceIntegrate(faceFlux*correction(vf))   to the div matrix,
 * i.e. source -= V*ivf (fvMatrix.C:1819-1826).  correction(vf) of linearUpwind (src/finiteVolume/interpolation/surfaceInterpolation/schemes/
 * linearUpwind/linearUpwind.C:33-62,65-199), on internal face f and component r:
 *     c = faceFlux[f] > 0 ? owner[f] : neighbour[f]     (STRICT; the weights use pos(), >= 0: at a zero flux the weight takes the owner,
 *                                                         the correction the neighbour)
 *     corr = (Cf[f] - C[c]) & grad_r[c]                 (the differences first; the dot product fma(dz, gz, fma(dx, gx, dy*gy)) as every
 *                                                         face pass of this engine; for a vector field vector & tensor component r)
 *     t_f  = faceFlux[f] * (scale*corr)                 (two stored fields, two roundings; scale 1: linearUpwind, 0.25: LUST, LUST.H:120-126)
 * and the weights: upwind (mi_upwind_weights / div_weights_dev NULL) for linearUpwind (linearUpwind.H:53-55), mi_lust_weights for LUST.
 * mi_div_correction: the correction's inputs; grad_dev[3*r + k] = d(vf_r)/dx_k, the cell gradient (e.g. mi_gauss_grad) of component r.
 * mi_linear_upwind_correction: t_f for n_rhs <= 4 components in ONE face pass over the internal faces (the reference: the correction
 *   field, [the scale,] the product, per component).  Then mi_surface_integrate(t, NULL, ivf) + the coupled patches' faces (below,
 *   mi_patch_add) + mi_vec_div(ivf, V) + mi_vec_submul(V, ivf, source) is the unfused sequence (without coupled patches
 *   mi_surface_integrate(t, V, ivf) divides in the same pass).
 * mi_patch_linear_upwind_correction: the same on one COUPLED patch (processor, cyclic; linearUpwind.C:49-62, the functor the reference
 *   runs): faceFlux > 0: (pCf - C[o]) & grad[o]; otherwise ((pCf - C[o]) - pd) & nbrGrad[i], o = faceCells[i], pd = patch().delta(),
 *   nbrGrad = the gradient's patchNeighbourField (mi_matrix_patch_neighbour_field per component).  Arrays: patch_cf / c / patch_delta 3
 *   component arrays each, grad / nbr_grad 3*n_rhs, out n_rhs.  Non-coupled patches contribute nothing.
 * mi_lust_weights: LUST.H:104-110, w = 0.75*cd_weights + 0.25*pos(faceFlux): three field operations, no fma.
 * mi_fvm_assemble_corrected: mi_fvm_assemble with that correction in the div term, in the same row pass: each block forms t_f of its own
 *   faces once and stages it in LDS; per cell ivf_r = (sum_own t - sum_nei t)/V (mi_surface_integrate's order), and
 *   source[r] = ((ddt source or 0.0) - V*ivf_r) before the su terms -- bit for bit the unfused sequence above placed after the ddt term.
 *   corr NULL: mi_fvm_assemble.  Refused (MI_ERR_ARG) without a convection term, and when the addressing has coupled patches
 *   (mi_addr_n_ext > 0): the reference adds those faces before the division by V, which only the unfused path reproduces.
 * Every call here rejects missing arrays, unaligned face fields and outputs that alias an input.                                   */
typedef struct mi_div_correction {
    double scale;                                  /* 1: linearUpwind, 0.25: LUST */
    const double *cf_dev[3];                       /* face centres Cf of the internal faces, component arrays (16-byte aligned) */
    const double *c_dev[3];                        /* cell centres C */
    const double *grad_dev[12];                    /* the first 3*n_rhs: grad_dev[3*r + k] = d(vf_r)/dx_k */
} mi_div_correction;
int mi_linear_upwind_correction(mi_addr_t addr, const mi_div_correction *corr, int32_t n_rhs, const double *face_flux_dev,
                                double *const *out_dev);
int mi_patch_linear_upwind_correction(mi_patch_t patch, double scale, int32_t n_rhs, const double *patch_flux_dev,
                                      const double *const *patch_cf_dev, const double *const *c_dev, const double *const *patch_delta_dev,
                                      const double *const *grad_dev, const double *const *nbr_grad_dev, double *const *out_dev);
int mi_lust_weights(mi_ctx_t ctx, int64_t n_faces, const double *cd_weights_dev, const double *face_flux_dev, double *weights_out_dev);
int mi_fvm_assemble_corrected(mi_addr_t addr, const mi_fvm_terms *terms, const mi_div_correction *corr_or_null,
                              double *lower_out_dev_or_null, double *upper_out_dev, double *diag_out_dev,
                              double *const *source_out_dev, double *sum_mag_off_diag_out_dev_or_null);
/* ---- explicit correction of the centred fourth-order scheme `Gauss cubic` ----
 * cubic<Type> is linear<Type> with corrected() true (src/finiteVolume/interpolation/surfaceInterpolation/schemes/cubic/cubic.H:104-107): the
 * weights are the linear ones (mesh.weights()), and gaussConvectionScheme::fvmDiv (gaussConvectionScheme.C:109-112) adds
 * fvc::surfaceIntegrate(faceFlux*correction(vf)), i.e. source -= V*ivf, exactly as it does for linearUpwind above.  correction(vf)
 * (cubic.H:111-184, the two-weight interpolate of surfaceInterpolationScheme.C:159-166,250-265), per face f from the one lambda = mesh.weights(),
 * every field operator rounded on its own:
 *     kSc   = lambda*(1 - lambda*(3 - 2*lambda))
 *     kVecP = ((1 - lambda)*(1 - lambda))*lambda
 *     kVecN = (lambda*lambda)*(lambda - 1)
 * and per component r (gaussGrad of vf.component(r): grad_dev[3*r + k] = d(vf_r)/dx_k, the Gauss linear cell gradient, e.g. mi_gauss_grad):
 *     c0   = fma(kSc, vf_r[P], (-kSc)*vf_r[N])                    (interpolate(vf, kSc, -kSc): the functor, first product fused)
 *     gI_k = fma(kVecP, grad_r,k[P], kVecN*grad_r,k[N])            (interpolate(grad, kVecP, kVecN), k = 0..2)
 *     corr = c0 + (((gI & Sf)/magSf)/deltaCoeffs)                 (gI & Sf = fma(gIz, Sfz, fma(gIx, Sfx, gIy*Sfy)))
 *     out  = faceFlux*corr, or corr itself when face_flux is NULL (fvc::interpolate under cubic: linear interpolate + corr)
 * mi_cubic_geometry: lambda = mesh.weights(), Sf (3 component arrays), magSf, surfaceInterpolation::deltaCoeffs() of the faces in question.
 * mi_cubic_correction: the internal faces, n_rhs <= 4 components in ONE face pass (the reference: about twenty per vector).
 * mi_patch_cubic_correction: one COUPLED patch (processor, or cyclic without rotation) with the patch's own lambda / Sf / magSf / deltaCoeffs:
 *   vf / grad through the patch's faceCells, nbr_vf / nbr_grad the patchNeighbourField (mi_matrix_patch_neighbour_field per array).  The
 *   reference evaluates a patch with field operators, so nothing but the dot product is contracted:
 *   c0 = kSc*pif + (-kSc)*pnf and gI_k = kVecP*g_k[o] + kVecN*nbr_g_k[i] are two rounded products and a sum.  Non-coupled patches take zero
 *   (cubic.H:175-181): no call is needed.
 * Into the matrix by the unfused route of linearUpwind: mi_fvm_div with the linear weights; mi_surface_integrate(t, ...) plus the coupled
 *   faces through mi_patch_add; mi_vec_submul(V, ivf, source).  mi_fvm_assemble_corrected and its time forms do NOT take cubic:
 *   mi_div_correction carries linearUpwind's inputs and is unchanged.
 * Both refuse (MI_ERR_ARG, nothing launched): n_rhs outside 1..4, a missing geometry / table / array, unaligned face fields (internal faces),
 *   an output that aliases an input or another output.                                                                              */
typedef struct mi_cubic_geometry {
    const double *lambda_dev;                      /* mesh.weights() */
    const double *sf_dev[3];                       /* Sf, component arrays */
    const double *mag_sf_dev;                      /* magSf */
    const double *delta_coeffs_dev;                /* surfaceInterpolation::deltaCoeffs() */
} mi_cubic_geometry;
int mi_cubic_correction(mi_addr_t addr, const mi_cubic_geometry *geo, int32_t n_rhs, const double *const *vf_dev,
                        const double *const *grad_dev, const double *face_flux_dev_or_null, double *const *out_dev);
int mi_patch_cubic_correction(mi_patch_t patch, const mi_cubic_geometry *patch_geo, int32_t n_rhs, const double *const *vf_dev,
                              const double *const *nbr_vf_dev, const double *const *grad_dev, const double *const *nbr_grad_dev,
                              const double *patch_flux_dev_or_null, double *const *out_dev);
/* ---- the backward time scheme: fvm::ddt, fvc::ddt, fvc::ddtCorr and the fused assembly ----
 * backwardDdtScheme<Type> (src/finiteVolume/finiteVolume/ddtSchemes/backwardDdtScheme/backwardDdtScheme.C), the static-mesh branches.  The
 * reference evaluates every expression below as field operators, one pass and one rounding per operator; the engine rounds every product,
 * sum and difference exactly as parenthesised here (no contraction), so the results equal the reference's bit for bit.
 * mi_ddt_backward_coeffs (host only, no device): backwardDdtScheme.C:472-479 with deltaT0_() of :57-69,
 *     coefft = 1 + deltaT/(deltaT + deltaT0);  coefft00 = deltaT*deltaT/(deltaT0*(deltaT + deltaT0));  coefft0 = coefft + coefft00
 *   coeffs_out = {coefft, coefft0, coefft00}.  n_old_times < 2 (the field has no old-old time yet): deltaT0 = GREAT = 1e15, which gives
 *   coefft = coefft0 = 1 and a coefft00 that is tiny but NOT zero -- the old-old field is always read; on the first step pass the old
 *   field for it (the reference creates oldTime().oldTime() as a copy).  MI_ERR_ARG: delta_t <= 0; delta_t0 <= 0 with n_old_times >= 2.
 * mi_fvm_ddt_backward: fvmDdt(vf) :456-504, fvmDdt(dimensionedScalar rho, vf) :507-553, fvmDdt(volScalarField rho, vf) :558-607
 *     rho_dev NULL:  diag = ((coefft*rDeltaT)*rho_value)*V;  source = ((rDeltaT*V)*rho_value)*((coefft0*psi0) - (coefft00*psi00))
 *     rho_dev given: diag = ((coefft*rDeltaT)*rho)*V;        source = (rDeltaT*V)*(((coefft0*rho0)*psi0) - ((coefft00*rho00)*psi00))
 *   (rho_value 1: fvm::ddt(vf)).  The three density arrays are given together or not at all.
 * mi_fvc_ddt_backward: fvcDdt(vf) :196-207, fvcDdt(dimensionedScalar rho, vf) :268-280, fvcDdt(volScalarField rho, vf) :343-355
 *     rho_dev NULL:  out = (rDeltaT*rho_value)*(((coefft*vf) - (coefft0*vf0)) + (coefft00*vf00))
 *     rho_dev given: out = rDeltaT*((((coefft*rho)*vf) - ((coefft0*rho0)*vf0)) + ((coefft00*rho00)*vf00))
 *   Both calls refuse (MI_ERR_ARG) a missing array, an unaligned array, and an output that is also an input or the other output.
 * mi_ddt_phi_corr_backward: fvcDdtPhiCorr(U, phi) :724-765 and fvcDdtPhiCorr(rho, U, phi) :868-950 (first branch) with
 *   ddtScheme<Type>::fvcDdtPhiCoeff (ddtSchemes/ddtScheme/ddtScheme.C:139-174), internal faces, ONE face pass:
 *     W = (coefft0*U0) - (coefft00*U00)  [with density (coefft0*(rho0*U0)) - (coefft00*(rho00*U00))], a cell field, rounded per cell
 *     k = 1 - min(|phi0 - flux(U0 or rho0*U0)|/(|phi0| + SMALL), 1)          (the OLD fields only)
 *     out = (k*rDeltaT)*(((coefft0*phi0) - (coefft00*phi00)) - flux(W)),   flux(X) = Sf & interpolate(X) as mi_flux_div forms it
 *   Each face gathers the old and old-old values of its two cells once and forms both fluxes from them.
 * mi_fvm_assemble_backward: mi_fvm_assemble / mi_fvm_assemble_corrected (corr_or_null) with the backward time derivative in the same row
 *   pass: terms->ddt != 0, terms->r_delta_t / rho_value / rho_dev / rho_old_dev / psi_old_dev keep their meaning, bw adds the coefficients
 *   and the old-old fields.  diag's time part and the start of every source are mi_fvm_ddt_backward's expressions; everything else (face
 *   terms, row sums, the correction, sp, su, sumMagOffDiag) is mi_fvm_assemble's -- so the outputs equal mi_fvm_ddt_backward + mi_fvm_div +
 *   mi_fvm_laplacian + the mi_vec_axpby combinations bit for bit.  MI_ERR_ARG: bw NULL, terms->ddt == 0, rho_old_old_dev given without
 *   rho_dev or the reverse, a missing old-old field; and every refusal of mi_fvm_assemble[_corrected].                                  */
typedef struct mi_ddt_backward {
    double coefft, coefft0, coefft00;              /* mi_ddt_backward_coeffs */
    const double *rho_old_old_dev;                 /* given exactly when terms->rho_dev is */
    const double *const *psi_old_old_dev;          /* n_rhs old-old fields */
} mi_ddt_backward;
int mi_ddt_backward_coeffs(double delta_t, double delta_t0, int32_t n_old_times, double coeffs_out[3]);
int mi_fvm_ddt_backward(mi_ctx_t ctx, int64_t n, double r_delta_t, const double coeffs[3], double rho_value, const double *rho_dev,
                        const double *rho_old_dev, const double *rho_old_old_dev, const double *vol_dev, const double *psi_old_dev,
                        const double *psi_old_old_dev, double *diag_out_dev, double *source_out_dev);
int mi_fvc_ddt_backward(mi_ctx_t ctx, int64_t n, double r_delta_t, const double coeffs[3], double rho_value, const double *rho_dev,
                        const double *rho_old_dev, const double *rho_old_old_dev, const double *vf_dev, const double *vf_old_dev,
                        const double *vf_old_old_dev, double *out_dev);
int mi_ddt_phi_corr_backward(mi_addr_t addr, double r_delta_t, const double coeffs[3], const double *lambda_dev, const double *sfx_dev,
                             const double *sfy_dev, const double *sfz_dev, const double *ux_old_dev, const double *uy_old_dev,
                             const double *uz_old_dev, const double *ux_old_old_dev, const double *uy_old_old_dev,
                             const double *uz_old_old_dev, const double *rho_old_dev_or_null, const double *rho_old_old_dev_or_null,
                             const double *phi_old_dev, const double *phi_old_old_dev, double *out_dev);
int mi_fvm_assemble_backward(mi_addr_t addr, const mi_fvm_terms *terms, const mi_ddt_backward *bw, const mi_div_correction *corr_or_null,
                             double *lower_out_dev_or_null, double *upper_out_dev, double *diag_out_dev, double *const *source_out_dev,
                             double *sum_mag_off_diag_out_dev_or_null);
/* ---- the CrankNicolson time scheme: the ddt0 state, fvm::ddt, fvc::ddt and the fused assembly ----
 * CrankNicolsonDdtScheme<Type> (src/finiteVolume/finiteVolume/ddtSchemes/CrankNicolsonDdtScheme/CrankNicolsonDdtScheme.{H,C}), the
 * !mesh().moving() branches.  The scheme carries STATE between time steps: ddt0(<name>), the previous step's time derivative, updated exactly
 * once per time step on first use, multiplied by the off-centring coefficient oc; the step on which it is first used is Euler's.  Every
 * expression below is evaluated by the reference as field operators, one pass and one rounding each; the engine rounds exactly as
 * parenthesised here (no contraction).  off(x) = (oc < 1) ? oc*x : x (offCentre_, .C:250-267).
 * NOT covered: the moving-mesh branches, the alpha*rho overloads, fvcDdtUfCorr, meshPhi; fvcDdt(dimensioned<Type>) (zero on a static mesh);
 *   reading or writing a ddt0(...) file for restarts (that needs ddt0's boundary field, which no engine operator forms: the state lives in
 *   memory for the run); icoFoam, which stays Euler-only.
 * mi_ddt_cn_parse (host only): exactly `CrankNicolson <oc>` with 0 <= oc <= 1 (the constructor's check, .H:165-180), any whitespace between
 *   and around.  MI_ERR_ARG with a message naming the token: a missing coefficient, an extra token, a non-number, NaN, oc outside [0, 1]
 *   ("should be >= 0 and <= 1"), any other scheme name, the empty string.
 * mi_ddt_cn_begin / mi_ddt_cn_step (host only): the DDt0Field's two time indices and the scalars of .C:186-247.
 *   begin(oc, time_index): the ddt0 field is created (zero -- the CALLER zeroes its arrays) at this time index: start_time_index =
 *   ddt0_time_index = time_index (ddt0_, .C:109-181).
 *   step(state, time_index, deltaT, deltaT0): evaluate = (ddt0_time_index != time_index);
 *       coef  = (time_index - start_time_index > 0) ? 1 + oc : 1;      r_dt_coef  = coef/deltaT     (one division)
 *       coef0 = (time_index - start_time_index > 1) ? 1 + oc : 1;      r_dt_coef0 = coef0/deltaT0   (0 for deltaT0 <= 0 without evaluate)
 *   and, when evaluate, ddt0_time_index = time_index -- the caller then runs mi_ddt_cn_update ONCE; a second step() in the same time step
 *   (non-orthogonal correctors) returns the same r_dt_coef with evaluate 0.  So: the first step is pure Euler with ddt0 untouched, the second
 *   has coef = 1 + oc, coef0 = 1, from the third on both are 1 + oc.  MI_ERR_ARG: deltaT <= 0; deltaT0 <= 0 when evaluate (read only then).
 * mi_ddt_cn_update: the ddt0 update (.C:417-418, :507-508, :603-607; the same statements in fvmDdt :818-822, :900-904, :987-994) of n_fields
 *   (1..4: the components of a vector) fields IN PLACE, one launch; element i of ddt0_inout_dev[k] is read and written by the same thread only
 *     rho_old_dev NULL:  ddt0 = ((rDtCoef0*rho_value)*(psi0 - psi00)) - off(ddt0)             (rho_value 1: the plain form)
 *     rho_old_dev given: ddt0 = (rDtCoef0*((rho0*psi0) - (rho00*psi00))) - off(ddt0)          (rho_old and rho_old_old together)
 * mi_fvm_ddt_cn: fvmDdt(vf) .C:755-832, fvmDdt(dimensionedScalar rho, vf) :837-913, fvmDdt(volScalarField rho, vf) :919-1003; ddt0_dev
 *   already updated for this time step
 *     rho_dev NULL:  diag = (rDtCoef*rho_value)*V;  source = (((rDtCoef*rho_value)*psi0) + off(ddt0))*V
 *     rho_dev given: diag = (rDtCoef*rho)*V;        source = (((rDtCoef*rho0)*psi0) + off(ddt0))*V       (rho and rho_old together)
 * mi_fvc_ddt_cn: fvcDdt(vf) .C:426, fvcDdt(dimensionedScalar rho, vf) :516, fvcDdt(volScalarField rho, vf) :615-616
 *     rho_dev NULL:  out = ((rDtCoef*rho_value)*(vf - vf0)) - off(ddt0)
 *     rho_dev given: out = (rDtCoef*((rho*vf) - (rho0*vf0))) - off(ddt0)
 *   The three device calls refuse (MI_ERR_ARG) a missing array, an unaligned array, an output that is also an input or another output, density
 *   arrays given partly, and oc outside [0, 1].
 * fvcDdtPhiCorr(U, phi) (.C:1164-1202) is Euler's expression with rDeltaT := rDtCoef: call mi_ddt_phi_corr with r_dt_coef.
 * mi_fvm_assemble_cn: mi_fvm_assemble / mi_fvm_assemble_corrected (corr_or_null) with the CrankNicolson time derivative in the same row pass:
 *   terms->ddt != 0 and terms->r_delta_t carries rDtCoef; cn = {oc, ddt0_dev[n_rhs]}.  diag's time part and the start of every source are
 *   mi_fvm_ddt_cn's expressions -- off(ddt0) is added BEFORE the multiplication by V, which no su term of mi_fvm_assemble can express --
 *   everything else is mi_fvm_assemble's, so the outputs equal mi_fvm_ddt_cn + mi_fvm_div + mi_fvm_laplacian + the mi_vec_axpby combinations
 *   bit for bit.  MI_ERR_ARG: cn NULL, terms->ddt == 0, a missing ddt0 array, a ddt0 array among the outputs, oc outside [0, 1]; and every
 *   refusal of mi_fvm_assemble[_corrected].                                                                                              */
typedef struct mi_ddt_cn_state {
    double oc;                                     /* the off-centring coefficient, 0 <= oc <= 1 */
    int32_t start_time_index, ddt0_time_index;     /* DDt0Field::startTimeIndex() and the ddt0 field's own timeIndex() */
} mi_ddt_cn_state;
typedef struct mi_ddt_cn_scalars {
    double r_dt_coef, r_dt_coef0;
    int32_t evaluate;                              /* 1: run mi_ddt_cn_update with r_dt_coef0 before any other use of ddt0 in this time step */
} mi_ddt_cn_scalars;
typedef struct mi_ddt_cn_terms {
    double oc;
    const double *const *ddt0_dev;                 /* n_rhs ddt0 fields, already updated for this time step */
} mi_ddt_cn_terms;
int mi_ddt_cn_parse(const char *scheme, double *oc_out);
int mi_ddt_cn_begin(double oc, int32_t time_index, mi_ddt_cn_state *state_out);
int mi_ddt_cn_step(mi_ddt_cn_state *state, int32_t time_index, double delta_t, double delta_t0, mi_ddt_cn_scalars *out);
int mi_ddt_cn_update(mi_ctx_t ctx, int64_t n, int32_t n_fields, double r_dt_coef0, double oc, double rho_value, const double *rho_old_dev,
                     const double *rho_old_old_dev, const double *const *psi_old_dev, const double *const *psi_old_old_dev,
                     double *const *ddt0_inout_dev);
int mi_fvm_ddt_cn(mi_ctx_t ctx, int64_t n, double r_dt_coef, double oc, double rho_value, const double *rho_dev, const double *rho_old_dev,
                  const double *vol_dev, const double *psi_old_dev, const double *ddt0_dev, double *diag_out_dev, double *source_out_dev);
int mi_fvc_ddt_cn(mi_ctx_t ctx, int64_t n, double r_dt_coef, double oc, double rho_value, const double *rho_dev, const double *rho_old_dev,
                  const double *vf_dev, const double *vf_old_dev, const double *ddt0_dev, double *out_dev);
int mi_fvm_assemble_cn(mi_addr_t addr, const mi_fvm_terms *terms, const mi_ddt_cn_terms *cn, const mi_div_correction *corr_or_null,
                       double *lower_out_dev_or_null, double *upper_out_dev, double *diag_out_dev, double *const *source_out_dev,
                       double *sum_mag_off_diag_out_dev_or_null);
/* ---- steadyState, the local-time-step schemes localEuler and CoEuler, and bounded Gauss convection ----
 * src/finiteVolume/finiteVolume/ddtSchemes/{steadyStateDdtScheme,localEulerDdtScheme,CoEulerDdtScheme} and convectionSchemes/
 * boundedConvectionScheme, the static-mesh branches.  Every expression is evaluated by the reference as field operators, one pass and one
 * rounding each; the engine rounds exactly as parenthesised here (no contraction).  max(a, b) = (a > b) ? a : b.  r = the rDeltaT CELL field.
 * NOT covered: SLTS, the `bounded` ddt scheme, the alpha*rho overloads, fvcDdtUfCorr, moving meshes, `bounded` together with the backward or
 *   CrankNicolson assembly forms.
 * steadyState: fvmDdt is an empty matrix, fvcDdt a zero field, fvcDdtPhiCorr a zero flux -- no call: leave the term out (terms->ddt == 0).
 * mi_ddt_local_parse (host only): `steadyState` | `localEuler <rDeltaT>` | `CoEuler <phi> <rho> <maxCo>`, any whitespace between and around.
 *   MI_ERR_ARG with a message naming the token: a missing or an extra word, a maxCo that is not a number, not finite or not > 0, `Euler` /
 *   `backward` / `CrankNicolson ...` ("not a local scheme"), any other name, a name longer than 63 characters, the empty string, NULL.
 * mi_fvm_ddt_local: fvmDdt of localEuler (localEulerDdtScheme.C:339-445) and of CoEuler with r = CorDeltaT() (CoEulerDdtScheme.C:459-606)
 *     rho_dev NULL:  diag = (r*rho_value)*V;  source = ((r*rho_value)*psi0)*V      (rho_value 1: fvm::ddt(vf), r*V and (r*psi0)*V)
 *     rho_dev given: diag = (r*rho)*V;        source = ((r*rho0)*psi0)*V           (rho and rho_old together)
 * mi_fvc_ddt_local: fvcDdt (:149-157, :200-209, :255-264; CoEuler :232-452)
 *     rho_dev NULL:  out = (r*rho_value)*(vf - vf0)
 *     rho_dev given: out = r*((rho*vf) - (rho0*vf0))
 *   Both refuse (MI_ERR_ARG) a missing or unaligned array, an output that is also an input or the other output, density arrays given partly.
 * mi_ddt_phi_corr_local: fvcDdtPhiCorr(U, phi) (:531-560; CoEuler :651-680), internal faces, one face pass: mi_ddt_phi_corr without density and
 *   with rDeltaT := fvc::interpolate(r) on the face, fma(lambda, r[P] - r[N], r[N]) (surfaceInterpolationScheme.C:275-280):
 *     out = ((1 - min(|phiCorr|/(|phi0| + SMALL), 1))*rDeltaT_f)*phiCorr,  phiCorr = phi0 - (Sf & interpolate(U0))
 *   The density forms fvcDdtPhiCorr(rho, U, phi) of both schemes (:653-726) use the GLOBAL 1/deltaT: that is mi_ddt_phi_corr.
 * mi_co_face_r_delta_t: CoEulerDdtScheme::CofrDeltaT (CoEulerDdtScheme.C:125-167) as a streaming pass over n faces (a patch's: the caller passes
 *   the patch's own deltaCoeffs, magSf, phi and -- mass flux -- the face density, the old density's boundary values)
 *     Co = (deltaCoeffs*(|phi|/magSf))*deltaT     [rho_face given: |phi|/(rho_face*magSf)];     out = max(Co/maxCo, 1.0)/deltaT
 * mi_co_r_delta_t: CoEulerDdtScheme::CorDeltaT (:61-94) on the internal faces in ONE row pass: out[c] = the maximum, from 0.0, of that face value
 *   over the cell's own faces, then its neighbour-side faces.  No face array is written.  lambda / rho_old given (together): the mass-flux form,
 *   rho_face = fvc::interpolate(rho.oldTime()) = fma(lambda, rho0[P] - rho0[N], rho0[N]) formed per face from the two cells.  A cell without
 *   internal faces gets 0.0 -- the patches follow (mi_patch_max per patch, in patch order; all values are positive, so the order is free).
 *   MI_ERR_ARG: deltaT or maxCo not positive and finite, lambda without rho_old or the reverse, the output among the inputs.
 * mi_patch_max (declared with mi_patch_add): cell_inout[faceCells[i]] = max(cell_inout[faceCells[i]], pf[i]) (matrixPatchOperation, :99-114).
 * mi_fvm_assemble_local: mi_fvm_assemble / mi_fvm_assemble_corrected (corr_or_null) with, in the same row pass,
 *   r_delta_t_dev given: the localEuler / CoEuler time derivative -- mi_fvm_ddt_local's expressions in place of Euler's; terms->ddt != 0 and
 *     terms->r_delta_t is ignored.  NULL: terms->ddt decides between Euler and no time derivative (steadyState), as in mi_fvm_assemble.
 *   div_flux_dev given: bounded Gauss convection (boundedConvectionScheme.C:69-92), fvmDiv = scheme.fvmDiv(flux, vf) - fvm::Sp(divPhi, vf) with
 *     divPhi = fvc::surfaceIntegrate(faceFlux) INCLUDING the boundary faces (mi_surface_integrate without volumes + mi_patch_add per patch +
 *     mi_vec_div): sumB' = sumB - (V*divPhi) -- the product rounded first (fvmSup.C:118), subtracted from the negSumDiag result
 *     (lduMatrixOperations.C:319-322) -- before sumB meets the time part.
 *   The outputs equal mi_fvm_ddt_local (or mi_fvm_ddt_euler*, or nothing) + mi_fvm_div [+ diag_div -= V*divPhi] + mi_fvm_laplacian + the
 *   mi_vec_axpby combinations bit for bit.  MI_ERR_ARG, nothing launched: loc NULL, both pointers NULL ("use mi_fvm_assemble"), r_delta_t_dev
 *   with terms->ddt == 0, div_flux_dev without terms->div_flux_dev, either array among the outputs; and every refusal of mi_fvm_assemble[_corrected]. */
#define MI_DDT_STEADY_STATE 0
#define MI_DDT_LOCAL_EULER 1
#define MI_DDT_CO_EULER 2
typedef struct mi_ddt_local_scheme {
    int32_t kind;                                  /* MI_DDT_STEADY_STATE | MI_DDT_LOCAL_EULER | MI_DDT_CO_EULER */
    char name[64];                                 /* localEuler: the rDeltaT field's name; CoEuler: the flux's name */
    char rho_name[64];                             /* CoEuler: the density's name (read for a mass flux) */
    double max_co;                                 /* CoEuler */
} mi_ddt_local_scheme;
typedef struct mi_fvm_local_terms {
    const double *r_delta_t_dev;                   /* n cells */
    const double *div_flux_dev;                    /* n cells: fvc::surfaceIntegrate(faceFlux) */
} mi_fvm_local_terms;
int mi_ddt_local_parse(const char *scheme, mi_ddt_local_scheme *out);
int mi_fvm_ddt_local(mi_ctx_t ctx, int64_t n, const double *r_delta_t_dev, double rho_value, const double *rho_dev, const double *rho_old_dev,
                     const double *vol_dev, const double *psi_old_dev, double *diag_out_dev, double *source_out_dev);
int mi_fvc_ddt_local(mi_ctx_t ctx, int64_t n, const double *r_delta_t_dev, double rho_value, const double *rho_dev, const double *rho_old_dev,
                     const double *vf_dev, const double *vf_old_dev, double *out_dev);
int mi_ddt_phi_corr_local(mi_addr_t addr, const double *r_delta_t_dev, const double *lambda_dev, const double *sfx_dev, const double *sfy_dev,
                          const double *sfz_dev, const double *ux_old_dev, const double *uy_old_dev, const double *uz_old_dev,
                          const double *phi_old_dev, double *out_dev);
int mi_co_face_r_delta_t(mi_ctx_t ctx, int64_t n, const double *delta_coeffs_dev, const double *mag_sf_dev, const double *phi_dev,
                         const double *rho_face_dev_or_null, double delta_t, double max_co, double *out_dev);
int mi_co_r_delta_t(mi_addr_t addr, const double *delta_coeffs_dev, const double *mag_sf_dev, const double *phi_dev,
                    const double *lambda_dev_or_null, const double *rho_old_dev_or_null, double delta_t, double max_co,
                    double *r_delta_t_out_dev);
int mi_fvm_assemble_local(mi_addr_t addr, const mi_fvm_terms *terms, const mi_fvm_local_terms *loc, const mi_div_correction *corr_or_null,
                          double *lower_out_dev_or_null, double *upper_out_dev, double *diag_out_dev, double *const *source_out_dev,
                          double *sum_mag_off_diag_out_dev_or_null);
/* fvMatrix::setReference (src/finiteVolume/fvMatrices/fvMatrix/fvMatrix.C:964-981; icoFoam.C:89, simpleFoam/pEqn.H:21: the pressure level of a
 * closed domain): source[celli] += diag[celli]*value; diag[celli] += diag[celli].  celli < 0 (the rank does not hold the cell): no-op. */
int mi_fvm_set_reference(mi_addr_t addr, int32_t celli, double value, double *diag_dev, double *source_dev);
/* fvMatrix::setValues (fvMatrix.C:454-656, functors :352-452; fvOptions constraints, wall-function cells): psi[cell] = value,
 * source[cell] = value*diag[cell]; the source of every OTHER row is corrected for its set neighbours; the coefficients that couple a
 * set row to its neighbours and the boundary coefficients of its patch faces are cleared.
 * upstream_semantics == 0, the REFERENCE's behaviour (it deviates from upstream OpenFOAM, SURVEY appendix B style): the correction uses
 * the transposed coefficient (lower[face] for an own face, upper[face] for a neighbour-side face), upper is cleared where the OWNER is
 * set and lower where the NEIGHBOUR is set, and a symmetric matrix comes out asymmetric (the reference's non-const lower() copies
 * upper) -- hence lower_out_dev is always written (lower_in_dev NULL: symmetric input).  != 0: upstream OpenFOAM's
 * (source[nei] -= lower*value, source[own] -= upper*value, both triangles cleared at every face of a set cell).  Outputs may alias inputs. */
int mi_fvm_set_values(mi_addr_t addr, int32_t n_set, const int32_t *cell_labels_dev, const double *values_dev, int32_t upstream_semantics,
                      double *psi_dev, const double *diag_dev, double *source_dev, const double *upper_in_dev, const double *lower_in_dev_or_null,
                      double *upper_out_dev, double *lower_out_dev, int32_t n_patches, const mi_patch_t *patches,
                      double *const *internal_coeffs_dev, double *const *boundary_coeffs_dev);
/* fvc::div(faceFlux, vf) -- gaussConvectionScheme<Type>::fvcDiv (src/finiteVolume/finiteVolume/convectionSchemes/gaussConvectionScheme/
 * gaussConvectionScheme.C:117-140): fvc::surfaceIntegrate(faceFlux*interpolate(faceFlux, vf)) on the internal faces; EEqn.H:9's fvc::div(phi, K).
 * weights NULL: upwind (pos(faceFlux)).  face_out receives faceFlux*interpolate (gaussConvectionScheme::flux, :62-70); div_out the row sums
 * [/ vol].  One face pass + one row pass (the reference: weights, interpolate, product, surfaceIntegrate = four field passes); boundary
 * faces: mi_patch_add on div_out as the reference adds them.                                                                           */
int mi_fvc_div(mi_addr_t addr, const double *face_flux_dev, const double *weights_dev_or_null, const double *vf_dev,
               const double *vol_dev_or_null, double *face_out_dev, double *div_out_dev);
/* out = x / y element-wise (fvMatrix::A = D/V, fvMatrix::H /= V; fvMatrix.C:1424-1506); out may alias x */
int mi_vec_div(mi_ctx_t ctx, int64_t n, const double *x_dev, const double *y_dev, double *out_dev);
/* Non-orthogonal correction of fvm::laplacian (row a22): gaussLaplacianScheme<Type, scalar>::fvmLaplacian with a `corrected`
 * snGrad scheme (laplacianSchemes/gaussLaplacianScheme/gaussLaplacianSchemes.C:64-90):
 *     source -= V * fvc::div( gammaMagSf * snGradScheme.correction(vf) ),
 * correction(vf) = nonOrthCorrectionVectors & linear.interpolate(grad(vf))  (snGradSchemes/correctedSnGrad/correctedSnGrad.C:45-65,
 * vectors of surfaceInterpolation.C:498-630: Sf/|Sf| - delta*nonOrthDeltaCoeffs on internal faces and coupled patches, zero on the others).
 * mi_sngrad_correction_flux is the face pass over the internal faces (the reference: an interpolated gradient field, a dot-product
 * field and a product field); mi_patch_sngrad_correction_flux the same on one COUPLED patch, with the patchNeighbourField of the gradient
 * (mi_matrix_patch_neighbour_field per component).  Then mi_surface_integrate(flux, NULL, div) + mi_patch_add(patch flux) + mi_vec_div(V)
 * is fvc::div and mi_vec_submul(V, div, source) the `source -= V*div`.  gamma_magsf NULL: the bare correction (snGrad, fvc::laplacian). */
int mi_sngrad_correction_flux(mi_addr_t addr, const double *corr_vec_x_dev, const double *corr_vec_y_dev, const double *corr_vec_z_dev,
                              const double *weights_dev, const double *grad_x_dev, const double *grad_y_dev, const double *grad_z_dev,
                              const double *gamma_magsf_dev_or_null, double *flux_out_dev);
int mi_patch_sngrad_correction_flux(mi_patch_t patch, const double *corr_vec_x_dev, const double *corr_vec_y_dev, const double *corr_vec_z_dev,
                                    const double *patch_weights_dev, const double *grad_x_dev, const double *grad_y_dev, const double *grad_z_dev,
                                    const double *nbr_grad_x_dev, const double *nbr_grad_y_dev, const double *nbr_grad_z_dev,
                                    const double *gamma_magsf_dev_or_null, double *flux_out_dev);
/* ---- the `limited` snGrad scheme (finiteVolume/snGradSchemes/limitedSnGrad/limitedSnGrad.{H,C}): `laplacianSchemes { default Gauss linear
 * limited 0.5; }`, `snGradSchemes { default limited corrected 0.33; }`.  correction(vf) = limiter * corr, with corr the `corrected` scheme's
 * correction per component (the value mi_sngrad_correction_flux forms with gamma_magsf NULL) and ONE limiter per face,
 *     limiter = min( k*mag(snGrad(vf)) / ((1 - k)*mag(corr) + SMALL), 1 )              (limitedSnGrad.C:58-84; SMALL = 1e-15),
 * snGrad = nonOrthDeltaCoeffs*(vf[N] - vf[P]) (snGradScheme.C:103-108), mag = fabs for a scalar, sqrt(magSqr) of the three components
 * for a vector.  k = 1 is `corrected` wherever |snGrad| >= SMALL, k = 0 `uncorrected`; neither is special-cased.
 * mi_sngrad_parse: host only, no GPU.  Accepts `uncorrected`, `orthogonal`, `corrected`, `limited <k>` (a number directly after the
 *   name: limitedSnGrad.H:86-97) and `limited corrected <k>`.  Refused (MI_ERR_ARG, the message names the token): k outside [0, 1], a
 *   missing or extra token, `limited uncorrected|orthogonal <k>` (their correction() is not implemented in the reference), `limited
 *   limited ...`, faceCorrected, linearFit, quadraticFit and unknown words.  limit_coeff is 1 for the kinds that do not read it.
 * mi_sngrad_limited_correction_flux: one face pass over the internal faces for n_comp = 1 (scalar) or 3 (vector) components:
 *   flux_out[j][f] = [gamma_magsf[f] *] (limiter[f] * corr_j[f]), every operation rounded where the reference's temporaries round it
 *   (DESIGN 3.5e); limiter_out (or NULL) receives the limiter.  vf_dev[n_comp], grad_dev[3*n_comp] (grad_dev[3*j + d] = d(vf_j)/dx_d, the
 *   full gradient as mi_gauss_grad + patches + /V leave it) and flux_out_dev[n_comp] are HOST arrays of device pointers.
 * mi_patch_sngrad_limited_correction_flux: the same on one COUPLED patch; corr as mi_patch_sngrad_correction_flux forms it, snGrad =
 *   patch_delta_coeffs*(nbr_vf - vf[faceCells]) (snGradScheme.C:165-169); nbr_vf / nbr_grad are the patchNeighbourFields
 *   (mi_matrix_patch_neighbour_field, transformed where the patch transforms).  Non-coupled patches carry zero correction vectors: no call.
 * Refused (MI_ERR_ARG, nothing launched): a missing array or one not aligned for a double, n_comp other than 1 or 3, limit_coeff
 *   outside [0, 1], an output that aliases an input or another output. */
enum { MI_SNGRAD_UNCORRECTED, MI_SNGRAD_ORTHOGONAL, MI_SNGRAD_CORRECTED, MI_SNGRAD_LIMITED };
typedef struct mi_sngrad_scheme {
    int32_t kind;          /* MI_SNGRAD_* */
    double limit_coeff;    /* k of the limited kind */
} mi_sngrad_scheme;
int mi_sngrad_parse(const char *text, mi_sngrad_scheme *out);
int mi_sngrad_limited_correction_flux(mi_addr_t addr, int32_t n_comp, double limit_coeff, const double *corr_vec_x_dev,
                                      const double *corr_vec_y_dev, const double *corr_vec_z_dev, const double *weights_dev,
                                      const double *delta_coeffs_dev, const double *const *vf_dev, const double *const *grad_dev,
                                      const double *gamma_magsf_dev_or_null, double *const *flux_out_dev, double *limiter_out_dev_or_null);
int mi_patch_sngrad_limited_correction_flux(mi_patch_t patch, int32_t n_comp, double limit_coeff, const double *corr_vec_x_dev,
                                            const double *corr_vec_y_dev, const double *corr_vec_z_dev, const double *patch_weights_dev,
                                            const double *patch_delta_coeffs_dev, const double *const *vf_dev,
                                            const double *const *nbr_vf_dev, const double *const *grad_dev,
                                            const double *const *nbr_grad_dev, const double *gamma_magsf_dev_or_null,
                                            double *const *flux_out_dev, double *limiter_out_dev_or_null);
/* ---- fvc::div(nuEff*dev(T(fvc::grad(U)))) and fvc::div(muEff*dev2(T(fvc::grad(U)))): the explicit term of divDevReff / divDevRhoReff
 * (incompressible laminar.C:202-225, compressible laminar.C:197, eddyViscosity.C:132).  grad[3*j + k] = d(U_j)/dx_k, nine
 * cell arrays (component j's mi_gauss_grad + patches + /V); kind MI_DEV (dev, coefficient 1.0/3.0) or MI_DEV2 (dev2, 2.0/3.0:
 * TensorI.H:534-546).  Per cell, every operation rounded as the reference's cell fields round it:
 *     tr = (grad[0] + grad[4]) + grad[8];  ii = coeff*tr;  X_kj = grad[3*k + j] - (k == j ? ii : 0);  Y_kj = visc*X_kj.
 * grad_dev, face_out_dev, div_out_dev and the other `const double *const *` arguments are HOST arrays of device pointers.
 * mi_fvc_div_dev_tgrad: the internal faces, one face pass (a face gathers the ten cell values of its two cells once) and one row pass
 *   for the three components:  I_kj = fma(lambda, Y_kj[P] - Y_kj[N], Y_kj[N]),  face_out[j] = fma(I_zj, Sf_z, fma(I_xj, Sf_x, I_yj*Sf_y)),
 *   div_out[j] = surfaceIntegrate(face_out[j]) [/ vol] in mi_surface_integrate's order -- bit for bit mi_flux_div(v = column j of X,
 *   cell_scale = visc).  `Vector & Tensor` is contracted per column as `Vector & Vector` is (an assumption: DESIGN 3.5a).  face_out is
 *   kept for the caller.  A case with patches passes vol NULL, adds the patch fluxes below with mi_patch_add in patch order, then mi_vec_div.
 *   Zero cells: MI_OK, nothing written.  Zero faces: MI_OK, div_out zeroed, the face arrays may be NULL.
 * mi_patch_gauss_grad_correct: the boundary values of a Gauss gradient on a patch that is NOT coupled (gaussGrad.C:277-303) for n_comp 1
 *   or 3:  n_k = Sf_k/magSf,  out[3*j + k] = g_k + n_k*(sngrad[j] - fma(n_z, g_z, fma(n_x, g_x, n_y*g_y))),  g = grad[3*j + .] at the
 *   face's cell (the zeroGradient value).  patch_sngrad[j]: the field's snGrad on the patch, deltaCoeffs*(U_b - U_internal) for a
 *   fixedValue patch, zeros for zeroGradient.  Outputs: 3*n_comp patch arrays.
 * mi_patch_dev_tgrad_flux: the three flux components on one patch's faces, flux[j] = Sf_b & column j of (visc*dev[2](T(G))).
 *   patch_weights NULL -- any patch that is not coupled: visc_dev and grad_dev[9] are the patch's own BOUNDARY values (patch arrays, e.g.
 *   from mi_patch_gauss_grad_correct); nbr_* are not read.  patch_weights given -- a coupled patch (processor; cyclic WITHOUT rotation):
 *   visc_dev and grad_dev[9] are the CELL arrays (read through faceCells), nbr_visc_dev / nbr_grad_dev[9] the patchNeighbourFields per
 *   patch face; Y is formed on each side and I = (w*Y_P) + ((1 - w)*Y_N), uncontracted.  A transforming (rotational) coupled patch is
 *   out of scope: the call does not transform the neighbour side.
 * Refused (MI_ERR_ARG, nothing launched, nothing written): a kind other than the two, n_comp other than 1 or 3, a missing array or one
 *   not aligned for a double, an output that aliases an input or another output. */
enum { MI_DEV, MI_DEV2 };
int mi_fvc_div_dev_tgrad(mi_addr_t addr, int32_t kind, const double *lambda_dev, const double *sfx_dev, const double *sfy_dev,
                         const double *sfz_dev, const double *visc_dev, const double *const *grad_dev, const double *vol_dev_or_null,
                         double *const *face_out_dev, double *const *div_out_dev);
int mi_patch_gauss_grad_correct(mi_patch_t patch, int32_t n_comp, const double *patch_sfx_dev, const double *patch_sfy_dev,
                                const double *patch_sfz_dev, const double *patch_magsf_dev, const double *const *patch_sngrad_dev,
                                const double *const *grad_dev, double *const *patch_grad_out_dev);
int mi_patch_dev_tgrad_flux(mi_patch_t patch, int32_t kind, const double *patch_sfx_dev, const double *patch_sfy_dev,
                            const double *patch_sfz_dev, const double *patch_weights_dev_or_null, const double *visc_dev,
                            const double *const *grad_dev, const double *nbr_visc_dev, const double *const *nbr_grad_dev,
                            double *const *flux_out_dev);
/* fvPatchField::patchInternalField: out[i] = psi[faceCells[i]] (zeroGradient boundary values for the Gauss gradient, fvMatrix::flux ...) */
int mi_patch_internal_field(mi_patch_t patch, const double *psi_dev, double *out_dev);
/* inout -= x*y, the product rounded before the subtraction (a temporary field, then operator-=) */
int mi_vec_submul(mi_ctx_t ctx, int64_t n, const double *x_dev, const double *y_dev, double *inout_dev);
int mi_patch_create(mi_ctx_t ctx, int32_t n_cells, int32_t n_patch_faces, const int32_t *face_cells_host, mi_patch_t *out);
int mi_patch_destroy(mi_patch_t patch);
int mi_patch_add(mi_patch_t patch, const double *pf_dev, double *intf_dev, int fn);
int mi_patch_max(mi_patch_t patch, const double *pf_dev, double *cell_inout_dev);   /* cell = max(cell, pf) per face cell (CoEuler, above) */
/* coupled part of fvMatrix::addBoundarySource (fvMatrix.C:318-346; used by fvMatrix::H, :1458-1506):
 * intf[faceCells[i]] +=(fn 0) / -=(fn 1) pf[i]*q[i], e.g. boundaryCoeffs * patchNeighbourField.            */
int mi_patch_add_product(mi_patch_t patch, const double *pf_dev, const double *q_dev, double *intf_dev, int fn);
/* boundary part of fvMatrix::flux (fvMatrix.C:1621-1653): flux[i] = internalCoeffs[i]*psi[faceCells[i]] -
 * boundaryCoeffs[i] * patchNeighbourField[i]  (coupled patch) | - boundaryCoeffs[i]  (NULL neighbour field: not coupled).
 * The internal-face part of flux() is mi_faceH.                                                                      */
int mi_patch_flux(mi_patch_t patch, const double *internal_coeffs_dev, const double *boundary_coeffs_dev,
                  const double *psi_dev, const double *patch_neighbour_field_dev_or_null, double *flux_dev);
/* fvMatrix<scalar>::relax(alpha) (fvMatrix.C:1087-1345, functors :983-1084): coupled[p] != 0 marks processor-like patches.
 * mi_relax_multi: the same for an equation with n_rhs sources / solution components that share the diagonal (fvMatrix<vector>::relax:
 * S += (D - D0)*psi per component); sum_mag_off_diag_dev_or_null: lduMatrix::sumMagOffDiag of the coefficients if the caller already
 * has it (mi_fvm_assemble's by-product; lower / upper may then be NULL) -- completed IN PLACE with the coupled patches' |boundaryCoeffs|. */
int mi_relax_multi(mi_addr_t addr, double alpha, double *diag_dev, const double *lower_dev, const double *upper_dev,
                   double *sum_mag_off_diag_dev_or_null, int32_t n_rhs, double *const *source_dev, const double *const *psi_dev,
                   int32_t n_patches, const mi_patch_t *patches, const double *const *internal_coeffs_dev,
                   const double *const *boundary_coeffs_dev, const int32_t *coupled);
int mi_relax(mi_addr_t addr, double alpha, double *diag_dev, const double *lower_dev, const double *upper_dev,
             double *source_dev, const double *psi_dev, int32_t n_patches, const mi_patch_t *patches,
             const double *const *internal_coeffs_dev, const double *const *boundary_coeffs_dev,
             const int32_t *coupled);

/* host-only inspection of the hierarchy builder (no device; CPU tests compare it with the
 * oracle's independent restatement).  name: restrictMap, faceRestrict, faceFlip (uint8), cLower,
 * cUpper, cellChildStart, cellChild, faceChildStart, faceChild, diagChildStart, diagChild.     */
int mi_gamg_host_build(int32_t n_cells, int32_t n_faces, const int32_t *lower_addr_host,
                       const int32_t *upper_addr_host, const double *face_weights_host,
                       int32_t n_cells_in_coarsest_level, int32_t merge_levels, int forward_init, void **hierarchy_out);
/* every domain of a DECOMPOSED case in one process (one thread per domain runs the per-rank builder, a barrier and a shared
 * table stand in for the communicator): patch p of domain d couples to patch patch_nbr_patch[d][p] of domain
 * patch_nbr_domain[d][p].  hierarchies_out[n_domains]; mi_gamg_host_patch_array: faceRestrict / faceCells / nbrCells of a
 * coupled patch on a level.  CPU tests compare with the oracle's multi-domain builder.                                  */
int mi_gamg_host_build_domains(int32_t n_domains, const int32_t *n_cells, const int32_t *n_faces,
                               const int32_t *const *lower_addr_host, const int32_t *const *upper_addr_host,
                               const double *const *face_weights_host, const int32_t *n_patches,
                               const int32_t *const *patch_sizes, const int32_t *const *const *patch_face_cells,
                               const int32_t *const *patch_nbr_domain, const int32_t *const *patch_nbr_patch,
                               int32_t n_cells_in_coarsest_level, int32_t merge_levels, int forward_init,
                               void **hierarchies_out);
/* one domain whose coupled patches are all cyclicAMI (arguments as mi_addr_set_ami_patch / mi_addr_set_ami_face_areas take
 * them, per patch); mi_gamg_host_patch_array then also answers "amiStart" / "amiAddr" (int32) and "amiW" / "amiMagSf" (double) */
int mi_gamg_host_build_ami(int32_t n_cells, int32_t n_faces, const int32_t *lower_addr_host, const int32_t *upper_addr_host,
                           const double *face_weights_host, int32_t n_cells_in_coarsest_level, int32_t n_patches,
                           const int32_t *patch_sizes, const int32_t *const *patch_face_cells_host, const int32_t *patch_nbr_patch,
                           const int32_t *const *ami_start_host, const int32_t *const *ami_addr_host, const double *const *ami_w_host,
                           const double *const *ami_mag_sf_host, void **hierarchy_out);
int mi_gamg_host_patch_array(void *hierarchy, int32_t level, int32_t patch, const char *name, const void **data,
                             int64_t *len);
int32_t mi_gamg_host_n_levels(void *hierarchy);
int mi_gamg_host_array(void *hierarchy, int32_t level, const char *name, const void **data,
                       int64_t *len, int32_t *elem_size);
int mi_gamg_host_free(void *hierarchy);

/* ---- distributed PCG (one rank per GPU).  The reference runs the same PCG on every
 * MPI rank and meets its neighbours in Foam::reduce (PCG.C:142,166,195 ->
 * src/Pstream/mpi/allReduceTemplates.C:195-208) and in the processor-patch exchange inside
 * Amul (lduMatrixUpdateMatrixInterfaces.C:30-276).  Here the device-resident pipeline is
 * cut at exactly those points: the caller owns the engine-order vectors (n_cells + n_ext
 * doubles each), an 8-double scalar block and the send buffer (n_ext doubles), runs the
 * collectives (RCCL through torch.distributed) between phases, and receives the halo
 * straight into pA[n_cells ..).  scal: [0] sum wA.rA  [1] sum|rA|  [2] sum wA.pA
 * [3] sum psi  [4] normFactor sum.  Phases:
 *    0  pack psi for the exchange            (then: exchange into psi ext)
 *    1  wA=A psi, rA, sumA, scal[3]          (then: allreduce scal[3]; avg = scal[3]/N_global)
 *    2  arg=avg: scal[4], scal[1], scal[0]   (then: allreduce scal[0..1], scal[4])
 *    3  normFactor, initial residual, first convergence test
 *   10  (test of it-1,) pA update, pack pA   (then: start exchange into pA ext)
 *   11  Amul interior tiles                  (overlaps the exchange)
 *   12  Amul boundary tiles, scal[2]         (after the exchange; then allreduce scal[2])
 *   13  psi, rA update, scal[1], scal[0]     (then: allreduce scal[0..1])
 *   14  convergence test of iteration `it`   (end of a batch)                           */
int mi_dpcg_set_buffers(mi_matrix_t m, double *psi_e, double *src_e, double *pA_e, double *wA_e,
                        double *rA_e, double *scal8, double *send_buf,
                        const mi_solver_controls *controls, int precond, int32_t history_len);
int mi_dpcg_phase(mi_matrix_t m, int phase, int32_t it, double arg);
int mi_dpcg_status(mi_matrix_t m, mi_solver_perf *perf_out, int32_t *done_out,
                   double *residual_history_host, int32_t history_len);
/* ---- RCCL communicator and the C++ host loop of the distributed PCG.  Replaces the reference's MPI layer
 * on this path (src/Pstream/mpi/UPstream.C, allReduceTemplates.C:195-208, UIPread.C/UOPwrite.C as used by
 * processorFvPatchScalarField.C:36-170): one rank per GPU, all-reduces on the engine's stream, halo
 * send/recv on a second stream so Amul's interior tiles overlap the exchange.  RCCL is bound at run time;
 * its absence is an error here (MI_ERR_DEVICE), never a fallback.
 *   id: 128 bytes from mi_comm_unique_id on rank 0, distributed to all ranks by the launcher (any channel).
 *   mi_dpcg_comm_begin: prologue up to the first convergence test (PCG.C:75-118); buffers and controls
 *     come from mi_dpcg_set_buffers.  reduce/halo may be the same communicator; two let the halo traffic
 *     and the scalar all-reduces progress independently.  patch_rank[p] = rank on the other side of
 *     processor patch p; patch_nbr_patch[p] = index of the matching patch on that rank (NULL = same index).
 *   mi_dpcg_comm_iterate: enqueue n_iters iterations without host synchronisation; poll with
 *     mi_dpcg_status.  record_amul_events = s > 0 brackets the Amul phases of every s-th enqueued iteration
 *     (k = 0, s, 2s, ...) with the events 2(k/s), 2(k/s)+1 of the matrix (mi_event_elapsed_ms).       */
int mi_comm_unique_id(void *id_out, int32_t len);
int mi_comm_create(mi_ctx_t ctx, int32_t n_ranks, int32_t rank, const void *id, mi_comm_t *out);
int mi_comm_destroy(mi_comm_t comm);
/* A communicator over the CALLER's transport instead of RCCL -- the reference's own is MPI through Pstream
 * (src/Pstream/mpi/UPstream.C:185-262 reduce, processorLduInterfaceTemplates.C:127-298 send/receive), so a shim inside a running
 * OpenFOAM application can hand its Pstream calls in here and needs no second launcher-level bootstrap.  Blocking by contract:
 * before every callback the engine synchronises the stream that produced the buffers; a callback returns (0 = ok) once its
 * results are in place in DEVICE memory.  allreduce: in-place sum over all ranks of n doubles.  exchange: one grouped
 * neighbour exchange (init/updateMatrixInterfaces): n_send messages (peer rank, tag, device pointer, count) and n_recv
 * messages; a message is matched by (peer, tag) -- the tag is the SENDER's patch index on both ends, so several patches per
 * peer and a rank that is its own neighbour work.  Everything the RCCL communicators do (attached operators and solvers,
 * mi_dpcg_comm_*, mi_gamg_create_coupled) runs over such a communicator too, without the compute/exchange overlap.          */
typedef int (*mi_comm_allreduce_fn)(void *user, double *buf_dev, int64_t n);
typedef int (*mi_comm_exchange_fn)(void *user, int32_t n_send, const int32_t *send_peer, const int32_t *send_tag,
                                   const double *const *send_dev, const int64_t *send_count, int32_t n_recv,
                                   const int32_t *recv_peer, const int32_t *recv_tag, double *const *recv_dev,
                                   const int64_t *recv_count);
int mi_comm_create_external(mi_ctx_t ctx, int32_t n_ranks, int32_t rank, mi_comm_allreduce_fn allreduce,
                            mi_comm_exchange_fn exchange, void *user, mi_comm_t *out);
int mi_comm_allreduce_sum(mi_comm_t comm, double *buf_dev, int64_t n);
/* Attach communicators to a matrix: from here on it behaves like the reference's lduMatrix on a decomposed
 * case -- mi_amul/tmul/residual/H/jacobi_smooth exchange the processor-patch values themselves
 * (init/updateMatrixInterfaces), every global sum inside the solvers is all-reduced, and
 * mi_pcg_solve / mi_pbicg_solve / mi_pbicgstab_solve / mi_smooth_solve solve the GLOBAL system; all ranks call
 * them together, like the MPI ranks of the reference.  (mi_pcg_solve: diagonal/none run the device-resident
 * phase pipeline, AINV a host-stepped loop.)  GAMG on such a matrix: mi_gamg_create_coupled.                 */
/* ONE-SHOT PEER ALL-REDUCE ("RCCL ncclAllReduce fallback / one-shot P2P all-to-all on the fully connected
 * node"; replaces the latency of src/Pstream/mpi/allReduceTemplates.C:195-208 for the 1-3 scalars of a Krylov iteration).
 * Opt-in, on any communicator (RCCL or external): every rank calls mi_comm_peer_window (allocates a window of device memory
 * -- fine-grained when the runtime exports that over IPC -- and returns its 64-byte hipIpcMemHandle), ships the handle to
 * all ranks with whatever transport it has, and calls mi_comm_peer_connect with the handles of ALL ranks in rank order;
 * after a barrier of the caller's, every all-reduce of <= 8 doubles on this communicator is one single-workgroup kernel
 * per rank: store the values + an epoch flag into the own slot of every rank's window, poll the own window until all
 * slots carry the epoch, add them in rank order (the same bits on every rank).  Larger all-reduces keep the
 * communicator's ordinary path.  mi_comm_peer_status: 0, or 1 once a wait has run out of polls (a rank that never
 * arrived: the sums are void); fine_grained_out says which memory the window got.  Exercised between processes that
 * share one device (tests/test_distributed.py); between devices it needs the fine-grained window -- unmeasured here. */
int mi_comm_peer_window(mi_comm_t comm, void *ipc_handle_out_64_bytes, int32_t len);
int mi_comm_peer_connect(mi_comm_t comm, const void *handles_rank_order, int32_t n_handles);
int mi_comm_peer_status(mi_comm_t comm, int32_t *status_out, int32_t *fine_grained_out_or_null);
/* The same set-up without help from the launcher, plus what makes it safe to be the DEFAULT (round 3):
 *   mi_comm_peer_auto     collective.  Allocates the window, all-gathers the IPC handles over the communicator's own transport
 *                         (RCCL or the external callbacks; the bytes travel as 16-bit integers through one all-reduce), maps the
 *                         peers, runs the coherence self-test and lets the ranks agree: *enabled_out = 1 on every rank, or 0 on
 *                         every rank (then nothing changes: RCCL / the external transport stay in charge).  It never fails because
 *                         windows are unavailable -- no IPC, a window that is not fine-grained while a peer sits on another device
 *                         (mi_comm_peer_connect refuses that with MI_ERR_UNSUPPORTED), a wait that runs out -- only on a broken
 *                         base transport.
 *   mi_comm_peer_selftest rounds all-reduces of known values against every peer with a short poll limit; *ok_out = 1 when every
 *                         sum is right.  All ranks together, after every rank has connected.
 *   mi_comm_peer_enable   switch the windows on / off after the ranks have agreed on the self-test's outcome.
 * A communicator in peer mode also moves the HALO of every matrix attached to it afterwards through windows
 * (mi_matrix_peer_halo_auto below), and the phase loop of the distributed PCG becomes three launches per iteration with no
 * collective call.  A wait that runs out of polls (a rank that died) raises a status word; the solver loops check it at their
 * host synchronisations and return MI_ERR_DEVICE (they used to carry on with void sums).                                      */
int mi_comm_peer_auto(mi_comm_t comm, int32_t *enabled_out);
int mi_comm_peer_selftest(mi_comm_t comm, int32_t rounds, int32_t *ok_out);
int mi_comm_peer_enable(mi_comm_t comm, int32_t on);
/* HALO WINDOWS (replaces lduMatrixUpdateMatrixInterfaces.C:30-276 / processorFvPatchScalarField.C:36-170 -- pack, host-staged
 * MPI_Isend/Irecv, unpack -- and this engine's own ncclSend/ncclRecv group): every attached matrix owns a window of
 * fine-grained device memory ([2 parities][n_ext] values + an epoch flag per patch and parity) that its neighbour ranks map
 * over hipIpc.  An exchange is then: one launch that gathers the patch-internal values and STORES them into the neighbours'
 * windows (k_halo_push; flags behind a system-scope release), the interior tiles meanwhile, one small launch that waits for the
 * own flags and copies the window into the operand's ext region (k_halo_pull; transformCoupleField factors of processorCyclic
 * patches applied there), the boundary tiles.  No second stream, no events, no collective call.  mi_matrix_attach_comm sets the
 * windows up by itself (collectively: every rank attaches its matching matrix at that point, GAMG level matrices included)
 * when the reduce communicator is in peer mode (MI_PEER_HALO=0 keeps the send/recv path); mi_matrix_peer_halo_auto does it
 * explicitly.  The set-up ends with a self-test against the communicator's ordinary exchange and an agreement of the ranks;
 * *enabled_out = 0 leaves the matrix on send/recv.  mi_matrix_peer_halo_status: whether windows are in use and whether a wait
 * has run out of polls.
 * With halo windows AND a peer-mode reduce communicator, mi_dpcg_comm_iterate (and mi_pcg_solve on the attached matrix,
 * diagonal / none) runs WITHOUT any collective call: k_dpcg_update_p (p-update + convergence test of the previous iteration +
 * deferred psi update; every block packs the patch cells of its own chunk into the neighbours' windows), tile_kernel_dist (all
 * tiles in one launch, interior first; block 0 raises the neighbours' flags, a boundary tile polls its own and reads the window
 * directly), a one-workgroup kernel that folds wA.pA and all-reduces it through the windows, k_dpcg_update_psi_r, a one-workgroup
 * kernel for sum|rA| and the next wA.rA: five launches, 51 us per iteration at 108^3 cells per rank against 81 us for the phase
 * loop over RCCL on the same box (profiles/r03_a_*; MI_DPCG_FUSED=0: the phase loop, 3 | 4: the all-reduces inside the passes,
 * measured slower).  The sums are formed in the order the separate reduction kernels use: same bits as the phase loop.
 * Not on this path: cyclicAMI / transformed patches (mi_dpcg_set_buffers refuses them: the boundary tiles read the window
 * without the interpolation / factor; mi_pcg_solve on such a matrix takes the tile-operator pipeline, whose k_halo_pull
 * applies the factors) and AINV (its preconditioner is itself a tile pass with a halo of its own).                              */
int mi_matrix_peer_halo_auto(mi_matrix_t m, int32_t *enabled_out);
int mi_matrix_peer_halo_status(mi_matrix_t m, int32_t *enabled_out, int32_t *status_out_or_null);
int mi_matrix_attach_comm(mi_matrix_t m, mi_comm_t reduce, mi_comm_t halo, const int32_t *patch_rank,
                          const int32_t *patch_nbr_patch_or_null, int64_t n_global_cells);
int mi_matrix_detach_comm(mi_matrix_t m);
/* coupledFvPatchField::patchNeighbourField (processorFvPatchField.C:107-135, cyclicFvPatchField.C:109-150): psi in the
 * cell across every interface face, n_ext values in caller patch order.  Cyclic patches read the partner cells;
 * processor patches exchange over the attached halo communicator (all ranks call together) -- what the coupled parts
 * of fvMatrix::flux / H consume (mi_patch_flux, mi_patch_add_product).                                           */
int mi_matrix_patch_neighbour_field(mi_matrix_t m, const double *psi_dev, double *nbr_out_dev);
int mi_dpcg_comm_begin(mi_matrix_t m, mi_comm_t reduce, mi_comm_t halo, const int32_t *patch_rank,
                       const int32_t *patch_nbr_patch_or_null, int64_t n_global_cells);
int mi_dpcg_comm_iterate(mi_matrix_t m, int32_t n_iters, int32_t record_amul_events);
/* HIP-event helpers on the context's stream (bench.py times the Amul phases with them) */
int mi_event_record(mi_matrix_t m, int32_t idx);
int mi_event_elapsed_ms(mi_matrix_t m, int32_t idx0, int32_t idx1, float *ms_out);

/* fvMatrix<vector>::solveSegregated (src/finiteVolume/fvMatrices/fvMatrix/fvMatrixSolve.C:103-225) as ONE call: nrhs <= 3
 * right-hand sides against the same matrix (the components of a momentum equation).  Every component runs the reference's
 * PBiCG loop (PBiCG.C:67-246) with its own scalars, convergence test and iteration count -- the same fma chains and reduction
 * trees as mi_pbicg_solve, hence the same bits per component -- while each pass over the matrix serves all components:
 * tile_kernel_multi stages a tile's upper / lower once for the 2 x nrhs operand vectors of a step (A pA_c and A^T pT_c; the
 * DILU pair precondition / preconditionT), sumA and 1/diag are computed once per coefficient binding, the host polls all
 * components with one copy.  diag_dev: nrhs device pointers to the components' DIAGONALS (caller order) -- solveSegregated adds
 * the boundary contribution per component, addBoundaryDiag(diag, cmpt), so the components share upper / lower but not
 * necessarily the diagonal -- or NULL: the bound diagonal for all.  psi_dev / source_dev: nrhs device pointers; perf_out: nrhs records;
 * residual_history_host: nrhs rows of history_len doubles (or NULL).  On a matrix with communicators attached (all ranks call
 * together) the shared passes stay: pA and pT of all components cross the processor patches in ONE halo exchange per pass, the
 * components' sums at a sum point travel in one all-reduce (round 4); only with cyclicAMI patches on an attached matrix are
 * the components solved one after the other.
 * mi_pbicg_solve itself uses the one-component form of the same kernel: A pA and A^T pT in one pass (MI_PBICG_PAIR=0: two).   */
int mi_pbicg_solve_multi(mi_matrix_t m, int32_t nrhs, const double *const *diag_dev_or_null, double *const *psi_dev, const double *const *source_dev,
                         const mi_solver_controls *controls, int precond, mi_solver_perf *perf_out,
                         double *residual_history_host, int32_t history_len);
int mi_pbicg_solve(mi_matrix_t m, double *psi_dev, const double *source_dev,
                   const mi_solver_controls *controls, int precond,
                   mi_solver_perf *perf_out, double *residual_history_host, int32_t history_len);
/* replicate_quirk != 0 keeps the reference's psi += omega*yA (PBiCGStab.C:263-270) */
int mi_pbicgstab_solve(mi_matrix_t m, double *psi_dev, const double *source_dev,
                       const mi_solver_controls *controls, int precond, int replicate_quirk,
                       mi_solver_perf *perf_out, double *residual_history_host, int32_t history_len);
int mi_smooth_solve(mi_matrix_t m, double *psi_dev, const double *source_dev,
                    const mi_solver_controls *controls, double omega, int32_t n_sweeps,
                    mi_solver_perf *perf_out, double *residual_history_host, int32_t history_len);

/* ---- benchmark hooks: run `iters` PCG iterations (engine order, no convergence
 * exit, same kernels as mi_pcg_solve) and `reps` Amuls back to back, timed with
 * HIP events on the context's stream; milliseconds returned.                      */
int mi_bench_amul(mi_matrix_t m, int32_t reps, float *ms_out);
/* diagnostic: resident Amul workgroups per CU as the HIP runtime computes it, LDS bytes per workgroup, block size */
int mi_debug_occupancy(mi_matrix_t m, int32_t *blocks_per_cu, int32_t *lds_bytes_out, int32_t *block_size);
/* diagnostic / test hook: the dense inversions behind GAMG's direct coarsest-level solve (GAMGSolverSolve.C:551-573: the reference
 * LU-solves the coarsest matrix on the host every cycle; the engine inverts it once per set of coefficients) on a row-major n x n
 * matrix in device memory.  which = 0 host Gauss-Jordan with partial pivoting, 1 / 2 the register-resident kernels (n <= 192; same
 * bits as 0), 3 the global-memory kernel.  *singular_out = 1: zero pivot column met.                                              */
int mi_debug_dense_invert(mi_ctx_t ctx, const double *a_dev, int32_t n, double *inv_dev, int32_t which, int32_t *singular_out);
int mi_bench_pcg_iters(mi_matrix_t m, const double *source_dev, int32_t iters, int precond,
                       float *ms_out, float *amul_ms_out);

/* ---- host-only layout inspection (no device; used by the CPU-side tests to
 * verify the tiling by interpreting the tables).  name is one of e2c, c2e,
 * tileCellStart, tileSlotStart, tileHaloStart, haloCell, tileSliceStart,
 * sliceEntryStart, entries (uint32), slotFace, extSlot, interiorTiles,
 * boundaryTiles, patchOffset, patchFaceCellsE, faceSlot (all int32 otherwise). */
int mi_layout_build_host(int32_t n_cells, int32_t n_faces, const int32_t *lower_addr_host,
                         const int32_t *upper_addr_host, int32_t n_patches, const int32_t *patch_sizes,
                         const int32_t *const *patch_face_cells_host,
                         const int32_t *const *patch_nbr_cells_host_or_null, int32_t tile_cells,
                         int32_t slot_cap, void **layout_out);
int mi_layout_array(void *layout, const char *name, const void **data, int64_t *len);
/* test hooks (round 4): the layout of a GIVEN partition (part[c] in [0, n_parts): tile of caller cell c; the partition of a
 * clustered layout gives that layout back), and the tiles a coarse GAMG level inherits from its fine level's tiles
 * (csrc/tiling.hpp inherit_tiles; part_out: n_coarse ids) */
int mi_layout_build_host_given(int32_t n_cells, int32_t n_faces, const int32_t *lower_addr_host, const int32_t *upper_addr_host,
                               int32_t n_parts, const int32_t *part_host, void **layout_out);
int mi_layout_inherit_tiles(int32_t n_fine, const int32_t *restrict_map, const int32_t *fine_tile_of_cell, int32_t n_fine_tiles,
                            int32_t n_coarse, int32_t n_coarse_faces, const int32_t *c_lower, const int32_t *c_upper,
                            int32_t cell_cap, int32_t slot_cap, int32_t *part_out, int32_t *n_parts_out);
int mi_layout_free(void *layout);

#ifdef __cplusplus
}
#endif
#endif /* MI_LDU_H */
