"""ctypes binding of the C ABI (include/mi_ldu.h) plus a thin object layer.

PyTorch is only plumbing here: device memory (``torch.Tensor.data_ptr()``),
the current HIP stream and ``torch.distributed``.  All arithmetic happens in
``librapidcfd_amd.so`` (hand-written gfx950 kernels).  There is no CPU
fallback: constructing a :class:`Context` without a gfx950 device raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librapidcfd_amd.so")
if os.environ.get("MI_ENGINE_LIB"):   # A/B builds of the engine (tools/ab_dma.sh); the product path is the in-tree library above
    LIB_PATH = os.environ["MI_ENGINE_LIB"]
_lib = None

PRECOND = {"none": 0, "diagonal": 1, "AINV": 2,
           # lduMatrixPreconditioner.C:58-61, DICPreconditioner.C:42-58: DIC/DILU resolve to AINV
           "DIC": 2, "DILU": 2, "FDIC": 2}


class MiError(RuntimeError):
    pass


class SolverPerf(C.Structure):
    _fields_ = [("initialResidual", C.c_double), ("finalResidual", C.c_double),
                ("normFactor", C.c_double), ("nIterations", C.c_int32),
                ("converged", C.c_int32), ("singular", C.c_int32), ("reserved", C.c_int32)]


class SolverControls(C.Structure):
    _fields_ = [("tolerance", C.c_double), ("relTol", C.c_double),
                ("maxIter", C.c_int32), ("minIter", C.c_int32)]


# every exported symbol of include/mi_ldu.h (tests check the library exports all of them)
SYMBOLS = [
    "mi_addr_set_ami_patch", "mi_addr_set_ami_patch_remote", "mi_addr_set_ami_face_areas", "mi_matrix_set_patch_transform",
    "mi_comm_peer_window", "mi_comm_peer_connect", "mi_comm_peer_status", "mi_gamg_create_dummy", "mi_gamg_host_build_ami",
    "mi_addr_create_adopted", "mi_layout_adopt_host", "mi_pbicg_solve_multi", "mi_comm_peer_auto", "mi_comm_peer_selftest", "mi_comm_peer_enable", "mi_matrix_peer_halo_auto", "mi_matrix_peer_halo_status",
    "mi_pcg_iterate_sampled", "mi_addr_set_ami_patch_remote_multi", "mi_fvm_assemble", "mi_fvm_set_reference", "mi_fvm_set_values", "mi_relax_multi", "mi_fvc_div",
    "mi_fvm_ddt_euler", "mi_fvm_ddt_euler_rho", "mi_fvm_su", "mi_fvm_sp", "mi_fvm_susp", "mi_flux_div", "mi_ddt_phi_corr", "mi_upwind_weights", "mi_limited_linear_weights", "mi_gauss_grad", "mi_vec_axpby", "mi_vec_div",
    "mi_comm_unique_id", "mi_comm_create", "mi_comm_destroy", "mi_comm_allreduce_sum", "mi_dpcg_comm_begin",
    "mi_dpcg_comm_iterate", "mi_gamg_create_coupled", "mi_matrix_attach_comm", "mi_matrix_detach_comm", "mi_matrix_patch_neighbour_field",
    "mi_ctx_create", "mi_ctx_destroy", "mi_ctx_synchronize", "mi_ctx_stat", "mi_ctx_set_option", "mi_last_error", "mi_device_available",
    "mi_addr_create", "mi_addr_create_coupled", "mi_addr_destroy", "mi_addr_n_cells", "mi_addr_n_faces", "mi_addr_n_tiles",
    "mi_addr_n_ext", "mi_addr_cell_perm", "mi_addr_stats", "mi_addr_patch_offsets",
    "mi_matrix_create", "mi_matrix_addr", "mi_matrix_destroy", "mi_matrix_set_coeffs", "mi_matrix_set_interface_coeffs",
    "mi_matrix_set_ext", "mi_halo_pack_engine", "mi_vec_to_engine", "mi_vec_from_engine",
    "mi_amul", "mi_tmul", "mi_sumA", "mi_residual", "mi_H", "mi_H1", "mi_faceH",
    "mi_amul_engine", "mi_tmul_engine", "mi_precondition", "mi_jacobi_smooth",
    "mi_sum", "mi_sum_prod", "mi_sum_mag", "mi_norm_factor", "mi_norm_factor_engine", "mi_precondition_engine",
    "mi_residual_engine", "mi_jacobi_smooth_engine",
    "mi_pcg_solve", "mi_pcg_begin", "mi_pcg_iterate", "mi_pcg_end",
    "mi_pbicg_solve", "mi_pbicgstab_solve", "mi_smooth_solve",
    "mi_bench_amul", "mi_bench_pcg_iters", "mi_debug_occupancy", "mi_debug_dense_invert",
    "mi_layout_build_host", "mi_layout_array", "mi_layout_free", "mi_layout_build_host_given", "mi_layout_inherit_tiles",
    "mi_dpcg_set_buffers", "mi_dpcg_phase", "mi_dpcg_status", "mi_event_record", "mi_event_elapsed_ms",
    "mi_gamg_create", "mi_gamg_update", "mi_gamg_level_matrix", "mi_gamg_scale", "mi_gamg_solve_coarsest", "mi_gamg_destroy", "mi_gamg_n_levels", "mi_gamg_forward_out", "mi_gamg_level_sizes",
    "mi_gamg_solve", "mi_gamg_restrict", "mi_gamg_prolong", "mi_gamg_level_coeffs",
    "mi_gamg_host_build", "mi_gamg_host_build_domains", "mi_gamg_host_patch_array", "mi_gamg_host_n_levels", "mi_gamg_host_array", "mi_gamg_host_free",
    "mi_row_face_op", "mi_fvm_laplacian", "mi_fvm_div", "mi_surface_integrate", "mi_face_interpolate",
    "mi_patch_create", "mi_patch_destroy", "mi_patch_add", "mi_patch_add_product", "mi_patch_flux", "mi_relax",
    "mi_sngrad_correction_flux", "mi_patch_sngrad_correction_flux", "mi_patch_internal_field", "mi_vec_submul",
    "mi_comm_create_external", "mi_addr_create_ordered", "mi_addr_tile_starts", "mi_addr_is_ordered",
    "mi_linear_upwind_correction", "mi_patch_linear_upwind_correction", "mi_lust_weights", "mi_fvm_assemble_corrected",
    "mi_limiter_parse", "mi_limited_weights", "mi_patch_limited_weights",
    "mi_filtered_parse", "mi_filtered_weights", "mi_patch_filtered_weights", "mi_cubic_correction", "mi_patch_cubic_correction",
    "mi_grad_limiter_parse", "mi_grad_boundary_create", "mi_grad_boundary_destroy", "mi_limited_grad",
    "mi_ddt_backward_coeffs", "mi_fvm_ddt_backward", "mi_fvc_ddt_backward", "mi_ddt_phi_corr_backward", "mi_fvm_assemble_backward",
    "mi_ddt_cn_parse", "mi_ddt_cn_begin", "mi_ddt_cn_step", "mi_ddt_cn_update", "mi_fvm_ddt_cn", "mi_fvc_ddt_cn", "mi_fvm_assemble_cn",
    "mi_ddt_local_parse", "mi_fvm_ddt_local", "mi_fvc_ddt_local", "mi_ddt_phi_corr_local", "mi_co_face_r_delta_t", "mi_co_r_delta_t", "mi_patch_max",
    "mi_fvm_assemble_local",
    "mi_sngrad_parse", "mi_sngrad_limited_correction_flux", "mi_patch_sngrad_limited_correction_flux",
    "mi_fvc_div_dev_tgrad", "mi_patch_gauss_grad_correct", "mi_patch_dev_tgrad_flux",
    "mi_grad_scheme_parse", "mi_ls_vectors_create", "mi_ls_vectors_destroy", "mi_ls_vectors_fields", "mi_ls_grad",
    "mi_surface_sum", "mi_reconstruct_create", "mi_reconstruct_destroy", "mi_reconstruct_fields", "mi_fvc_reconstruct",
    "mi_mules_create", "mi_mules_destroy", "mi_mules_work", "mi_mules_begin", "mi_mules_iterate", "mi_mules_apply", "mi_mules_limiter", "mi_mules_limit",
    "mi_mules_explicit_solve", "mi_vec_min",
    "mi_mules_begin_corr", "mi_mules_limiter_corr", "mi_mules_limit_corr", "mi_mules_correct",
    "mi_interface_compression_parse", "mi_interface_compression_weights", "mi_patch_interface_compression_weights",
    "mi_alpha_compression_flux", "mi_patch_alpha_compression_flux",
    "mi_interface_nhatf", "mi_patch_interface_nhatf", "mi_interface_create", "mi_interface_destroy", "mi_interface_curvature",
    "mi_surface_tension_force", "mi_patch_surface_tension_force", "mi_near_interface",
    "mi_ke_coeffs_init", "mi_min_max", "mi_vec_max_value", "mi_average_create", "mi_average_destroy", "mi_fvc_average", "mi_bound",
    "mi_ke_production", "mi_ke_create", "mi_ke_destroy", "mi_ke_wall_cells", "mi_ke_wall_cell_labels", "mi_ke_wall_values",
    "mi_ke_epsilon_terms", "mi_ke_k_terms", "mi_ke_nut", "mi_ke_nut_wall",
    "mi_sst_coeffs_init", "mi_sst_production", "mi_sst_wall_cells", "mi_sst_blend", "mi_sst_omega_sources", "mi_sst_k_terms", "mi_sst_nut",
    "mi_thermo_model_init", "mi_thermo_calculate", "mi_thermo_calculate_boundary", "mi_thermo_he", "mi_thermo_property",
    "mi_central_scheme_parse", "mi_central_flux", "mi_patch_central_flux", "mi_central_sound_speed", "mi_central_courant",
    "mi_les_coeffs_init", "mi_les_simple_filter", "mi_les_delta_cube_root_vol", "mi_les_smagorinsky", "mi_les_k_terms", "mi_les_nusgs",
    "mi_les_dyn_moments", "mi_les_dyn_level1", "mi_les_dyn_level2", "mi_les_dyn_coeffs",
    "mi_sa_coeffs_init", "mi_sa_terms", "mi_sa_nut", "mi_sa_nut_spalding_wall",
]


class GamgControls(C.Structure):
    _fields_ = [("tolerance", C.c_double), ("relTol", C.c_double), ("maxIter", C.c_int32), ("minIter", C.c_int32),
                ("nPreSweeps", C.c_int32), ("preSweepsLevelMultiplier", C.c_int32), ("maxPreSweeps", C.c_int32),
                ("nPostSweeps", C.c_int32), ("postSweepsLevelMultiplier", C.c_int32), ("maxPostSweeps", C.c_int32),
                ("nFinestSweeps", C.c_int32), ("scaleCorrection", C.c_int32), ("omega", C.c_double),
                ("directSolveCoarsest", C.c_int32), ("reserved", C.c_int32)]


def gamg_controls(tolerance=1e-6, relTol=0.0, maxIter=1000, minIter=0, nPreSweeps=0, preSweepsLevelMultiplier=1,
                  maxPreSweeps=4, nPostSweeps=2, postSweepsLevelMultiplier=1, maxPostSweeps=4, nFinestSweeps=2,
                  scaleCorrection=-1, omega=0.9, directSolveCoarsest=True):
    """GAMGSolver.C:67-77 defaults"""
    return GamgControls(tolerance, relTol, maxIter, minIter, nPreSweeps, preSweepsLevelMultiplier, maxPreSweeps,
                        nPostSweeps, postSweepsLevelMultiplier, maxPostSweeps, nFinestSweeps, scaleCorrection, omega,
                        int(bool(directSolveCoarsest)), 0)


def adopt_host(n_cells, lower_addr, upper_addr, patch_face_cells=(), patch_nbr_cells=()):
    """host part of renumber-at-bind (mi_layout_adopt_host): dict with cell_map, face_map, face_flipped, lower, upper, n_tiles"""
    lo = np.ascontiguousarray(lower_addr, dtype=np.int32); up = np.ascontiguousarray(upper_addr, dtype=np.int32)
    patches = [np.ascontiguousarray(p, dtype=np.int32) for p in patch_face_cells]
    npatch = len(patches)
    I32, U8 = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    sizes = (C.c_int32 * max(npatch, 1))(*[p.shape[0] for p in patches])
    ptrs = (I32 * max(npatch, 1))(*[p.ctypes.data_as(I32) for p in patches])
    nbrs = [None if (k >= len(patch_nbr_cells) or patch_nbr_cells[k] is None) else np.ascontiguousarray(patch_nbr_cells[k], dtype=np.int32) for k in range(npatch)]
    nptrs = (I32 * max(npatch, 1))(*[q.ctypes.data_as(I32) if q is not None else I32() for q in nbrs])
    out = dict(cell_map=np.empty(n_cells, dtype=np.int32), face_map=np.empty(lo.shape[0], dtype=np.int32), face_flipped=np.empty(lo.shape[0], dtype=np.uint8),
               lower=np.empty(lo.shape[0], dtype=np.int32), upper=np.empty(lo.shape[0], dtype=np.int32))
    nt = C.c_int32(0)
    _chk(lib().mi_layout_adopt_host(C.c_int32(n_cells), C.c_int32(lo.shape[0]), lo.ctypes.data_as(I32), up.ctypes.data_as(I32), C.c_int32(npatch), sizes, ptrs, nptrs,
                                    out["cell_map"].ctypes.data_as(I32), out["face_map"].ctypes.data_as(I32), out["face_flipped"].ctypes.data_as(U8),
                                    out["lower"].ctypes.data_as(I32), out["upper"].ctypes.data_as(I32), C.byref(nt)))
    out["n_tiles"] = int(nt.value)
    return out


def host_layout(n_cells, lower_addr, upper_addr, patch_face_cells=(), tile_cells=0, slot_cap=0, patch_nbr_cells=()) -> dict:
    """Build the tiled layout on the host only and return its tables as numpy arrays (tests)."""
    lo = np.ascontiguousarray(lower_addr, dtype=np.int32)
    up = np.ascontiguousarray(upper_addr, dtype=np.int32)
    patches = [np.ascontiguousarray(p, dtype=np.int32) for p in patch_face_cells]
    npatch = len(patches)
    sizes = (C.c_int32 * max(npatch, 1))(*[p.shape[0] for p in patches])
    ptrs = (C.POINTER(C.c_int32) * max(npatch, 1))(*[p.ctypes.data_as(C.POINTER(C.c_int32)) for p in patches])
    h = C.c_void_p()
    nbrs = [None if (k >= len(patch_nbr_cells) or patch_nbr_cells[k] is None)
            else np.ascontiguousarray(patch_nbr_cells[k], dtype=np.int32) for k in range(npatch)]
    nptrs = (C.POINTER(C.c_int32) * max(npatch, 1))(*[q.ctypes.data_as(C.POINTER(C.c_int32)) if q is not None
                                                       else C.POINTER(C.c_int32)() for q in nbrs])
    _chk(lib().mi_layout_build_host(C.c_int32(n_cells), C.c_int32(lo.shape[0]),
                                    lo.ctypes.data_as(C.POINTER(C.c_int32)), up.ctypes.data_as(C.POINTER(C.c_int32)),
                                    C.c_int32(npatch), sizes, ptrs, nptrs, C.c_int32(tile_cells), C.c_int32(slot_cap), C.byref(h)))
    out = {}
    try:
        for name in ("e2c", "c2e", "tileCellStart", "tileSlotStart", "tileIfaceSlot0", "tileHaloStart", "haloCell",
                     "tileSliceStart", "sliceEntryStart", "entries", "slotFace", "extSlot", "interiorTiles", "boundaryTiles",
                     "patchOffset", "patchFaceCellsE", "faceSlot", "sliceEntryStart16", "entries16", "slotBase", "tileSbStart"):
            data, ln = C.c_void_p(), C.c_int64()
            _chk(lib().mi_layout_array(h, name.encode(), C.byref(data), C.byref(ln)))
            dt = np.uint32 if name in ("entries", "entries16") else (np.uint16 if name == "slotBase" else np.int32)
            if ln.value:
                buf = (C.c_char * (ln.value * np.dtype(dt).itemsize)).from_address(data.value)
                out[name] = np.frombuffer(buf, dtype=dt).copy()
            else:
                out[name] = np.zeros(0, dtype=dt)
    finally:
        lib().mi_layout_free(h)
    return out


_LAYOUT_ARRAYS = ("e2c", "c2e", "tileCellStart", "tileSlotStart", "tileIfaceSlot0", "tileHaloStart", "haloCell", "tileSliceStart", "sliceEntryStart",
                  "entries", "slotFace", "extSlot", "interiorTiles", "boundaryTiles", "patchOffset", "patchFaceCellsE", "faceSlot")


def host_layout_given(n_cells, lower_addr, upper_addr, part, n_parts) -> dict:
    """Host-only layout of a GIVEN partition (mi_layout_build_host_given; tests)."""
    I32 = C.POINTER(C.c_int32)
    lo = np.ascontiguousarray(lower_addr, dtype=np.int32); up = np.ascontiguousarray(upper_addr, dtype=np.int32)
    pt = np.ascontiguousarray(part, dtype=np.int32)
    h = C.c_void_p()
    _chk(lib().mi_layout_build_host_given(C.c_int32(n_cells), C.c_int32(lo.shape[0]), lo.ctypes.data_as(I32), up.ctypes.data_as(I32), C.c_int32(n_parts), pt.ctypes.data_as(I32), C.byref(h)))
    out = {}
    try:
        for name in _LAYOUT_ARRAYS:
            data, ln = C.c_void_p(), C.c_int64()
            _chk(lib().mi_layout_array(h, name.encode(), C.byref(data), C.byref(ln)))
            dt = np.uint32 if name == "entries" else np.int32
            out[name] = np.frombuffer((C.c_char * (ln.value * 4)).from_address(data.value), dtype=dt).copy() if ln.value else np.zeros(0, dtype=dt)
    finally:
        lib().mi_layout_free(h)
    return out


def inherit_tiles(restrict_map, fine_tile_of_cell, n_fine_tiles, n_coarse, c_lower, c_upper, cell_cap=0, slot_cap=0):
    """Tiles of a coarse GAMG level inherited from its fine level's tiles (mi_layout_inherit_tiles; tests): (part, n_parts)."""
    I32 = C.POINTER(C.c_int32)
    rm = np.ascontiguousarray(restrict_map, dtype=np.int32); ft = np.ascontiguousarray(fine_tile_of_cell, dtype=np.int32)
    cl = np.ascontiguousarray(c_lower, dtype=np.int32); cu = np.ascontiguousarray(c_upper, dtype=np.int32)
    part = np.empty(n_coarse, dtype=np.int32); n_parts = C.c_int32()
    _chk(lib().mi_layout_inherit_tiles(C.c_int32(rm.shape[0]), rm.ctypes.data_as(I32), ft.ctypes.data_as(I32), C.c_int32(n_fine_tiles), C.c_int32(n_coarse),
                                       C.c_int32(cl.shape[0]), cl.ctypes.data_as(I32), cu.ctypes.data_as(I32), C.c_int32(cell_cap), C.c_int32(slot_cap),
                                       part.ctypes.data_as(I32), C.byref(n_parts)))
    return part, int(n_parts.value)


def lib():
    """Load the native library; fail loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MiError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'`")
        # PyTorch (the plumbing for device memory / streams here) preloads its bundled HIP runtime by path.  If the engine
        # were loaded first it would bind /opt/rocm's copy, torch would then map a second runtime, and the second one
        # cannot open the device ("no ROCm-capable device").  Loading torch first makes both share one runtime.
        try:
            import torch  # noqa: F401
        except ImportError:  # pure C-ABI use without PyTorch
            pass
        _lib = C.CDLL(LIB_PATH)
        _lib.mi_last_error.restype = C.c_char_p
    return _lib


def _chk(rc: int):
    if rc != 0:
        raise MiError(f"mi error {rc}: {lib().mi_last_error().decode()}")


def device_available() -> bool:
    return bool(lib().mi_device_available())


def _ptr(t) -> C.c_void_p:
    """Device pointer of a contiguous float64 torch tensor (or None)."""
    if t is None:
        return C.c_void_p(0)
    assert t.is_contiguous() and t.dtype.is_floating_point and t.element_size() == 8, "need contiguous float64"
    return C.c_void_p(t.data_ptr())


def _ptrs(xs, least=1):
    """The device pointers of a list of tensors as a C array of at least `least` entries, NULL past the list (or None for None)."""
    return None if xs is None else (C.c_void_p * max(len(xs), least))(*[_ptr(x) for x in xs])


class Context:
    def __init__(self, device: int = 0, stream_handle: Optional[int] = None):
        self.h = C.c_void_p()
        _chk(lib().mi_ctx_create(int(device), C.c_void_p(stream_handle or 0), C.byref(self.h)))
        self.device = device

    def synchronize(self):
        _chk(lib().mi_ctx_synchronize(self.h))

    def set_option(self, name: str, value: int):
        """mi_ctx_set_option: "pcg_persist", "pcg_fuse_rp", "win_direct", "gamg_graph_attached" 0 / 1"""
        _chk(lib().mi_ctx_set_option(self.h, name.encode(), C.c_int32(int(value))))

    def dense_invert(self, a_dev, inv_dev, n: int, which: int) -> bool:
        """diagnostic: invert the row-major n x n matrix a_dev into inv_dev with path `which` (mi_debug_dense_invert); False: singular"""
        sing = C.c_int32()
        _chk(lib().mi_debug_dense_invert(self.h, _ptr(a_dev), C.c_int32(n), _ptr(inv_dev), C.c_int32(which), C.byref(sing)))
        return sing.value == 0

    def stat(self, which: int) -> int:
        """mi_ctx_stat: 0 = launches of the persistent PCG kernel on plain matrices, 1 = on communicator-attached ones,
        2 = grid-barrier litmus runs, 3 = V-cycles of a decomposed case replayed as a hipGraph, 4 = launches of the fused residual / direction kernel of PCG,
        5 = batches of PCG iterations replayed as a hipGraph (mi_pcg_solve), PBiCG loops run through 6 = the multi-vector solver,
        7 = pbicg_solve_device (once per component), 8 = the host-stepped loop (MI_PBICG_HOST_STEPPED), PBiCGStab solves through
        9 = the device loop (pbicgstab_solve_device), 10 = the host-stepped loop, 11 = PBiCGStab solves that ended at the mid-iteration exit,
        12 = tile launches that took the persistent walk (MI_TILE_PERSIST: fewer workgroups than tiles).
        (6, 7 and 9 are bodies enqueued by the one batch driver of csrc/engine.hip, drive_batches.)"""
        v = C.c_int64(0)
        _chk(lib().mi_ctx_stat(self.h, C.c_int32(which), C.byref(v)))
        return int(v.value)

    def close(self):
        if self.h:
            lib().mi_ctx_destroy(self.h)
            self.h = C.c_void_p()

    # field reductions -------------------------------------------------------
    def _red(self, fn, a, b=None):
        out = C.c_double()
        if b is None:
            _chk(getattr(lib(), fn)(self.h, _ptr(a), C.c_int64(a.numel()), C.byref(out)))
        else:
            _chk(getattr(lib(), fn)(self.h, _ptr(a), _ptr(b), C.c_int64(a.numel()), C.byref(out)))
        return out.value

    def sum(self, a):
        return self._red("mi_sum", a)

    def sum_mag(self, a):
        return self._red("mi_sum_mag", a)

    def sum_prod(self, a, b):
        return self._red("mi_sum_prod", a, b)


class Addressing:
    """lduAddressing: host lowerAddr/upperAddr + coupled-patch faceCells -> tiled engine layout."""

    def __init__(self, ctx: Context, n_cells: int, lower_addr, upper_addr, patch_face_cells: Sequence = (),
                 patch_nbr_cells: Sequence = (), ordered: bool = False, tile_cell_start=None, adopt: bool = False):
        """patch_nbr_cells[p] (optional): local cells across patch p => cyclic (local) coupling; None => processor patch.
        ordered: keep the caller's numbering (mi_addr_create_ordered); tile_cell_start: the tiles as cell ranges, or None.
        adopt: renumber-at-bind (mi_addr_create_adopted) -- the addressing is that of the mesh RENUMBERED into the engine order;
        self.cell_map / face_map / face_flipped / lower_addr / upper_addr describe the renumbering (new -> old)"""
        self.ctx = ctx
        lo = np.ascontiguousarray(lower_addr, dtype=np.int32)
        up = np.ascontiguousarray(upper_addr, dtype=np.int32)
        self._patches = [np.ascontiguousarray(p, dtype=np.int32) for p in patch_face_cells]
        npatch = len(self._patches)
        sizes = (C.c_int32 * max(npatch, 1))(*[p.shape[0] for p in self._patches])
        ptrs = (C.POINTER(C.c_int32) * max(npatch, 1))(*[p.ctypes.data_as(C.POINTER(C.c_int32)) for p in self._patches])
        self.h = C.c_void_p()
        self._nbrs = [None if (k >= len(patch_nbr_cells) or patch_nbr_cells[k] is None)
                      else np.ascontiguousarray(patch_nbr_cells[k], dtype=np.int32) for k in range(npatch)]
        nptrs = (C.POINTER(C.c_int32) * max(npatch, 1))(*[q.ctypes.data_as(C.POINTER(C.c_int32)) if q is not None
                                                           else C.POINTER(C.c_int32)() for q in self._nbrs])
        if adopt:
            I32, U8 = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
            self.cell_map = np.empty(n_cells, dtype=np.int32); self.face_map = np.empty(lo.shape[0], dtype=np.int32)
            self.face_flipped = np.empty(lo.shape[0], dtype=np.uint8)
            self.lower_addr = np.empty(lo.shape[0], dtype=np.int32); self.upper_addr = np.empty(lo.shape[0], dtype=np.int32)
            _chk(lib().mi_addr_create_adopted(ctx.h, C.c_int32(n_cells), C.c_int32(lo.shape[0]), lo.ctypes.data_as(I32), up.ctypes.data_as(I32),
                                              C.c_int32(npatch), sizes, ptrs, nptrs, self.cell_map.ctypes.data_as(I32), self.face_map.ctypes.data_as(I32),
                                              self.face_flipped.ctypes.data_as(U8), self.lower_addr.ctypes.data_as(I32), self.upper_addr.ctypes.data_as(I32),
                                              C.byref(self.h)))
        elif ordered:
            ts = None if tile_cell_start is None else np.ascontiguousarray(tile_cell_start, dtype=np.int32)
            _chk(lib().mi_addr_create_ordered(ctx.h, C.c_int32(n_cells), C.c_int32(lo.shape[0]),
                                              lo.ctypes.data_as(C.POINTER(C.c_int32)), up.ctypes.data_as(C.POINTER(C.c_int32)),
                                              C.c_int32(npatch), sizes, ptrs, nptrs, C.c_int32(0 if ts is None else ts.shape[0] - 1),
                                              ts.ctypes.data_as(C.POINTER(C.c_int32)) if ts is not None else C.POINTER(C.c_int32)(), C.byref(self.h)))
        else:
            _chk(lib().mi_addr_create_coupled(ctx.h, C.c_int32(n_cells), C.c_int32(lo.shape[0]),
                                              lo.ctypes.data_as(C.POINTER(C.c_int32)), up.ctypes.data_as(C.POINTER(C.c_int32)),
                                              C.c_int32(npatch), sizes, ptrs, nptrs, C.byref(self.h)))
        self.n_cells = n_cells
        self.n_faces = int(lo.shape[0])
        self.n_ext = int(lib().mi_addr_n_ext(self.h))
        self.n_tiles = int(lib().mi_addr_n_tiles(self.h))

    def cell_perm(self) -> np.ndarray:
        out = np.empty(self.n_cells, dtype=np.int32)
        _chk(lib().mi_addr_cell_perm(self.h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def tile_starts(self) -> np.ndarray:
        out = np.empty(self.n_tiles + 1, dtype=np.int32)
        _chk(lib().mi_addr_tile_starts(self.h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    @property
    def is_ordered(self) -> bool:
        return bool(lib().mi_addr_is_ordered(self.h))

    def set_ami_patch(self, patch: int, nbr_patch: int, start=None, address=None, weights=None, low_weight=None):
        """patch becomes a cyclicAMI patch coupled to nbr_patch (mi_addr_set_ami_patch); start None: one face to one face with
        unit weights (a cyclic patch that carries a transformation factor)"""
        ip = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
        st, ad = ip(start), ip(address)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        lw = None if low_weight is None else np.ascontiguousarray(low_weight, dtype=np.uint8)
        cp = lambda a, t: a.ctypes.data_as(C.POINTER(t)) if a is not None else None
        _chk(lib().mi_addr_set_ami_patch(self.h, C.c_int32(patch), C.c_int32(nbr_patch), cp(st, C.c_int32), cp(ad, C.c_int32),
                                         cp(w, C.c_double), cp(lw, C.c_uint8)))

    def set_ami_patch_remote(self, patch: int, transport_patch: int, n_partner_faces: int, start, address, weights, low_weight=None):
        """cyclicAMI patch whose partner lives on another rank: its neighbour values are interpolated from what the processor
        patch `transport_patch` receives (mi_addr_set_ami_patch_remote)"""
        st = np.ascontiguousarray(start, dtype=np.int32); ad = np.ascontiguousarray(address, dtype=np.int32)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        lw = None if low_weight is None else np.ascontiguousarray(low_weight, dtype=np.uint8)
        _chk(lib().mi_addr_set_ami_patch_remote(self.h, C.c_int32(patch), C.c_int32(transport_patch), C.c_int32(n_partner_faces),
                                                st.ctypes.data_as(C.POINTER(C.c_int32)), ad.ctypes.data_as(C.POINTER(C.c_int32)),
                                                w.ctypes.data_as(C.POINTER(C.c_double)),
                                                lw.ctypes.data_as(C.POINTER(C.c_uint8)) if lw is not None else C.POINTER(C.c_uint8)()))

    def set_ami_patch_remote_multi(self, patch: int, transport_patches, n_partner_faces, start, address, weights, low_weight=None):
        """cyclicAMI patch whose partner SIDE is split over several ranks: one transport patch per partner piece, addresses numbering the
        pieces' faces concatenated (mi_addr_set_ami_patch_remote_multi)"""
        tp = np.ascontiguousarray(transport_patches, dtype=np.int32); nf = np.ascontiguousarray(n_partner_faces, dtype=np.int32)
        st = np.ascontiguousarray(start, dtype=np.int32); ad = np.ascontiguousarray(address, dtype=np.int32)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        lw = None if low_weight is None else np.ascontiguousarray(low_weight, dtype=np.uint8)
        I32 = C.POINTER(C.c_int32)
        _chk(lib().mi_addr_set_ami_patch_remote_multi(self.h, C.c_int32(patch), C.c_int32(tp.shape[0]), tp.ctypes.data_as(I32), nf.ctypes.data_as(I32),
                                                      st.ctypes.data_as(I32), ad.ctypes.data_as(I32), w.ctypes.data_as(C.POINTER(C.c_double)),
                                                      lw.ctypes.data_as(C.POINTER(C.c_uint8)) if lw is not None else C.POINTER(C.c_uint8)()))

    def set_ami_face_areas(self, patch: int, mag_sf):
        """face areas of a cyclicAMI patch (srcMagSf / tgtMagSf): the GAMG hierarchy agglomerates the AMI with them"""
        a = np.ascontiguousarray(mag_sf, dtype=np.float64)
        _chk(lib().mi_addr_set_ami_face_areas(self.h, C.c_int32(patch), a.ctypes.data_as(C.POINTER(C.c_double))))

    def patch_offsets(self) -> np.ndarray:
        out = np.empty(len(self._patches) + 1, dtype=np.int32)
        _chk(lib().mi_addr_patch_offsets(self.h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def stats(self) -> dict:
        st = (C.c_int64 * 8)()
        _chk(lib().mi_addr_stats(self.h, st))
        keys = ["tiles", "slots", "entries", "halo", "max_cells", "max_slots", "max_halo", "lds_bytes_sym"]
        return dict(zip(keys, [int(v) for v in st]))

    def to_engine(self, x, out):
        _chk(lib().mi_vec_to_engine(self.h, _ptr(x), _ptr(out)))

    def from_engine(self, xe, out):
        _chk(lib().mi_vec_from_engine(self.h, _ptr(xe), _ptr(out)))

    def halo_pack(self, xe, send):
        _chk(lib().mi_halo_pack_engine(self.h, _ptr(xe), _ptr(send)))

    def close(self):
        if self.h:
            lib().mi_addr_destroy(self.h)
            self.h = C.c_void_p()


class Comm:
    """RCCL communicator of one rank (mi_comm_*).  ``unique_id()`` on rank 0, ship the 128 bytes to every rank."""

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_char * 128)()
        _chk(lib().mi_comm_unique_id(buf, C.c_int32(128)))
        return bytes(buf)

    def __init__(self, ctx: "Context", n_ranks: int, rank: int, uid: bytes):
        self.ctx = ctx
        self.h = C.c_void_p()
        self.n_ranks, self.rank = n_ranks, rank
        _chk(lib().mi_comm_create(ctx.h, C.c_int32(n_ranks), C.c_int32(rank), C.c_char_p(uid), C.byref(self.h)))

    def allreduce_sum(self, t):
        _chk(lib().mi_comm_allreduce_sum(self.h, _ptr(t), C.c_int64(t.numel())))

    # one-shot peer all-reduce (opt-in): window() on every rank, ship the 64 bytes to all ranks, peer_connect(all handles)
    def peer_window(self) -> bytes:
        buf = (C.c_char * 64)()
        _chk(lib().mi_comm_peer_window(self.h, buf, C.c_int32(64)))
        return bytes(buf)

    def peer_connect(self, handles):
        blob = b"".join(handles)
        assert len(blob) == 64 * self.n_ranks
        _chk(lib().mi_comm_peer_connect(self.h, C.c_char_p(blob), C.c_int32(self.n_ranks)))

    def peer_status(self):
        st, fg = C.c_int32(0), C.c_int32(0)
        _chk(lib().mi_comm_peer_status(self.h, C.byref(st), C.byref(fg)))
        return int(st.value), bool(fg.value)

    def peer_auto(self) -> bool:
        """collective: windows + handle exchange over the communicator's own transport + self-test + agreement (mi_comm_peer_auto);
        True on every rank when the scalars (and the halo of matrices attached afterwards) travel through peer windows"""
        on = C.c_int32(0)
        _chk(lib().mi_comm_peer_auto(self.h, C.byref(on)))
        return bool(on.value)

    def peer_selftest(self, rounds: int = 16) -> bool:
        ok = C.c_int32(0)
        _chk(lib().mi_comm_peer_selftest(self.h, C.c_int32(rounds), C.byref(ok)))
        return bool(ok.value)

    def peer_enable(self, on: bool):
        _chk(lib().mi_comm_peer_enable(self.h, C.c_int32(1 if on else 0)))

    def close(self):
        if self.h:
            lib().mi_comm_destroy(self.h)
            self.h = C.c_void_p()


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                          C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_void_p), C.POINTER(C.c_int64))


class ExternalComm(Comm):
    """A communicator over the CALLER's transport (mi_comm_create_external) -- MPI through Pstream in an OpenFOAM shim, gloo
    in the tests.  ``allreduce(ptr, n)`` sums n doubles at device pointer ptr over the ranks in place; ``exchange(sends, recvs)``
    gets lists of (peer, tag, device pointer, count) and returns when the received data is in device memory."""

    def __init__(self, ctx: "Context", n_ranks: int, rank: int, allreduce, exchange):
        self.ctx = ctx
        self.h = C.c_void_p()
        self.n_ranks, self.rank = n_ranks, rank
        self.errors = []

        def _ar(_user, buf, n):
            try:
                allreduce(int(buf), int(n)); return 0
            except Exception as e:  # an exception must not unwind through the C frames
                self.errors.append(e); return 1

        def _ex(_user, ns, sp, st, sb, sc, nr, rp, rt, rb, rc):
            try:
                exchange([(sp[i], st[i], int(sb[i]), int(sc[i])) for i in range(ns)], [(rp[i], rt[i], int(rb[i]), int(rc[i])) for i in range(nr)]); return 0
            except Exception as e:
                self.errors.append(e); return 1

        self._cb = (ALLREDUCE_FN(_ar), EXCHANGE_FN(_ex))      # keep the trampolines alive as long as the communicator
        _chk(lib().mi_comm_create_external(ctx.h, C.c_int32(n_ranks), C.c_int32(rank), self._cb[0], self._cb[1], None, C.byref(self.h)))


class Matrix:
    """lduMatrix coefficients bound to an :class:`Addressing`."""

    def __init__(self, addr: Addressing):
        self.addr = addr
        self.h = C.c_void_p()
        _chk(lib().mi_matrix_create(addr.h, C.byref(self.h)))

    def set_coeffs(self, diag, upper, lower=None):
        _chk(lib().mi_matrix_set_coeffs(self.h, _ptr(diag), _ptr(upper), _ptr(lower)))

    def set_interface_coeffs(self, patch: int, bou, inte=None):
        _chk(lib().mi_matrix_set_interface_coeffs(self.h, C.c_int32(patch), _ptr(bou), _ptr(inte)))

    def set_patch_transform(self, patch: int, factor: float):
        """transformCoupleField factor of a coupled patch (mi_matrix_set_patch_transform)"""
        _chk(lib().mi_matrix_set_patch_transform(self.h, C.c_int32(patch), C.c_double(factor)))

    def set_ext(self, ext):
        _chk(lib().mi_matrix_set_ext(self.h, _ptr(ext)))

    # SpMV family (caller order) ---------------------------------------------
    def amul(self, psi, out):
        _chk(lib().mi_amul(self.h, _ptr(psi), _ptr(out)))

    def tmul(self, psi, out):
        _chk(lib().mi_tmul(self.h, _ptr(psi), _ptr(out)))

    def sumA(self, out):
        _chk(lib().mi_sumA(self.h, _ptr(out)))

    def residual(self, psi, source, out):
        _chk(lib().mi_residual(self.h, _ptr(psi), _ptr(source), _ptr(out)))

    def H(self, psi, out):
        _chk(lib().mi_H(self.h, _ptr(psi), _ptr(out)))

    def H1(self, out):
        _chk(lib().mi_H1(self.h, _ptr(out)))

    def patch_neighbour_field(self, psi, out):
        """psi across every interface face (n_ext values, caller patch order); exchanges when a communicator is attached"""
        _chk(lib().mi_matrix_patch_neighbour_field(self.h, _ptr(psi), _ptr(out)))

    def norm_factor(self, psi, source, Apsi):
        out = C.c_double(0.0)
        _chk(lib().mi_norm_factor(self.h, _ptr(psi), _ptr(source), _ptr(Apsi), C.byref(out)))
        return out.value

    def faceH(self, psi, out):
        _chk(lib().mi_faceH(self.h, _ptr(psi), _ptr(out)))

    # engine order -------------------------------------------------------------
    def amul_engine(self, psi_e, out_e, which: int = 0):
        _chk(lib().mi_amul_engine(self.h, _ptr(psi_e), _ptr(out_e), int(which)))

    def tmul_engine(self, psi_e, out_e, which: int = 0):
        _chk(lib().mi_tmul_engine(self.h, _ptr(psi_e), _ptr(out_e), int(which)))

    def precondition(self, kind: str, rA, wA, transpose: bool = False):
        _chk(lib().mi_precondition(self.h, PRECOND[kind], int(transpose), _ptr(rA), _ptr(wA)))

    def jacobi_smooth(self, psi, source, n_sweeps: int, omega: float = 0.9):
        _chk(lib().mi_jacobi_smooth(self.h, C.c_double(omega), _ptr(psi), _ptr(source), C.c_int32(n_sweeps)))

    # solvers -------------------------------------------------------------------
    def _solve(self, fn, psi, source, extra, tolerance, relTol, maxIter, minIter):
        ctl = SolverControls(tolerance, relTol, maxIter, minIter)
        perf = SolverPerf()
        hist_len = maxIter + 2
        hist = np.full(hist_len, np.nan)
        _chk(getattr(lib(), fn)(self.h, _ptr(psi), _ptr(source), C.byref(ctl), *extra, C.byref(perf),
                                hist.ctypes.data_as(C.POINTER(C.c_double)), C.c_int32(hist_len)))
        out = {k: getattr(perf, k) for k, _ in SolverPerf._fields_ if k != "reserved"}
        out["history"] = hist[~np.isnan(hist)].copy()
        return out

    def pcg(self, psi, source, precond="diagonal", tolerance=1e-6, relTol=0.0, maxIter=1000, minIter=0):
        return self._solve("mi_pcg_solve", psi, source, (C.c_int(PRECOND[precond]),), tolerance, relTol, maxIter, minIter)

    def pbicg(self, psi, source, precond="diagonal", tolerance=1e-6, relTol=0.0, maxIter=1000, minIter=0):
        return self._solve("mi_pbicg_solve", psi, source, (C.c_int(PRECOND[precond]),), tolerance, relTol, maxIter, minIter)

    def pbicg_multi(self, psis, sources, precond="diagonal", tolerance=1e-6, relTol=0.0, maxIter=1000, minIter=0, diags=None):
        """the components of a vector equation in one solve (mi_pbicg_solve_multi): list of per-component results;
        diags: per-component diagonals (addBoundaryDiag(diag, cmpt)) or None = the bound diagonal for all"""
        n = len(psis)
        assert 1 <= n <= 3 and len(sources) == n
        ctl = SolverControls(tolerance, relTol, maxIter, minIter)
        perf = (SolverPerf * n)()
        hist_len = maxIter + 2
        hist = np.full((n, hist_len), np.nan)
        P = (C.c_void_p * n)(*[_ptr(t) for t in psis])
        S = (C.c_void_p * n)(*[_ptr(t) for t in sources])
        D = None if diags is None else (C.c_void_p * n)(*[_ptr(t) for t in diags])
        _chk(lib().mi_pbicg_solve_multi(self.h, C.c_int32(n), D, P, S, C.byref(ctl), C.c_int(PRECOND[precond]), perf,
                                        hist.ctypes.data_as(C.POINTER(C.c_double)), C.c_int32(hist_len)))
        out = []
        for k in range(n):
            d = {f: getattr(perf[k], f) for f, _ in SolverPerf._fields_ if f != "reserved"}
            d["history"] = hist[k][~np.isnan(hist[k])].copy()
            out.append(d)
        return out

    def pbicgstab(self, psi, source, precond="diagonal", tolerance=1e-6, relTol=0.0, maxIter=1000, minIter=0,
                  replicate_quirk=True):
        return self._solve("mi_pbicgstab_solve", psi, source, (C.c_int(PRECOND[precond]), C.c_int(int(replicate_quirk))),
                           tolerance, relTol, maxIter, minIter)

    def smooth_solve(self, psi, source, n_sweeps=1, omega=0.9, tolerance=1e-6, relTol=0.0, maxIter=1000, minIter=0):
        return self._solve("mi_smooth_solve", psi, source, (C.c_double(omega), C.c_int32(n_sweeps)),
                           tolerance, relTol, maxIter, minIter)

    # PCG session (bench) -------------------------------------------------------
    def pcg_begin(self, psi0, source, precond="diagonal", tolerance=0.0, relTol=0.0, maxIter=1000, minIter=0,
                  history_len=0):
        ctl = SolverControls(tolerance, relTol, maxIter, minIter)
        _chk(lib().mi_pcg_begin(self.h, _ptr(psi0), _ptr(source), C.byref(ctl), C.c_int(PRECOND[precond]),
                                C.c_int32(history_len)))

    def pcg_iterate(self, n_iters: int, time_amul: bool = False, event_stride: int = 1) -> Optional[float]:
        if time_amul:
            ms = C.c_float()
            _chk(lib().mi_pcg_iterate_sampled(self.h, C.c_int32(n_iters), C.c_int32(event_stride), C.byref(ms)))
            return ms.value
        _chk(lib().mi_pcg_iterate(self.h, C.c_int32(n_iters), None))
        return None

    def pcg_end(self, psi_out=None, history_len=0):
        perf = SolverPerf()
        hist = np.full(max(history_len, 1), np.nan)
        _chk(lib().mi_pcg_end(self.h, _ptr(psi_out), C.byref(perf), hist.ctypes.data_as(C.POINTER(C.c_double)),
                              C.c_int32(history_len)))
        out = {k: getattr(perf, k) for k, _ in SolverPerf._fields_ if k != "reserved"}
        out["history"] = hist[: min(history_len, perf.nIterations + 1)].copy()
        return out

    # distributed PCG phases (parallel.py) -----------------------------------------
    def dpcg_set_buffers(self, psi_e, src_e, pA_e, wA_e, rA_e, scal8, send_buf, precond="diagonal",
                         tolerance=0.0, relTol=0.0, maxIter=1000, minIter=0, history_len=0):
        ctl = SolverControls(tolerance, relTol, maxIter, minIter)
        _chk(lib().mi_dpcg_set_buffers(self.h, _ptr(psi_e), _ptr(src_e), _ptr(pA_e), _ptr(wA_e), _ptr(rA_e),
                                       _ptr(scal8), _ptr(send_buf), C.byref(ctl), C.c_int(PRECOND[precond]),
                                       C.c_int32(history_len)))

    def dpcg_phase(self, phase: int, it: int = 0, arg: float = 0.0):
        _chk(lib().mi_dpcg_phase(self.h, int(phase), C.c_int32(it), C.c_double(arg)))

    def dpcg_status(self, history_len=0):
        perf = SolverPerf()
        done = C.c_int32()
        hist = np.full(max(history_len, 1), np.nan)
        _chk(lib().mi_dpcg_status(self.h, C.byref(perf), C.byref(done), hist.ctypes.data_as(C.POINTER(C.c_double)),
                                  C.c_int32(history_len)))
        out = {k: getattr(perf, k) for k, _ in SolverPerf._fields_ if k != "reserved"}
        out["done"] = int(done.value)
        out["history"] = hist[~np.isnan(hist)].copy()
        return out

    def attach_comm(self, reduce: "Comm", halo: "Comm", patch_rank, patch_nbr_patch=None, n_global=0):
        """decomposed-case behaviour for every operator and solver of this matrix (mi_matrix_attach_comm)"""
        pr = np.ascontiguousarray(patch_rank, dtype=np.int32)
        pn = None if patch_nbr_patch is None else np.ascontiguousarray(patch_nbr_patch, dtype=np.int32)
        I32 = C.POINTER(C.c_int32)
        _chk(lib().mi_matrix_attach_comm(self.h, reduce.h, halo.h, pr.ctypes.data_as(I32) if pr.size else I32(),
                                         pn.ctypes.data_as(I32) if pn is not None and pn.size else I32(), C.c_int64(n_global)))
        self._comms = (reduce, halo)

    def detach_comm(self):
        _chk(lib().mi_matrix_detach_comm(self.h))
        self._comms = None

    def peer_halo_auto(self) -> bool:
        """collective: halo windows of this attached matrix (mi_matrix_peer_halo_auto); True when every rank has them"""
        on = C.c_int32(0)
        _chk(lib().mi_matrix_peer_halo_auto(self.h, C.byref(on)))
        return bool(on.value)

    def peer_halo_status(self):
        """(windows in use, a wait ran out of polls)"""
        on, st = C.c_int32(0), C.c_int32(0)
        _chk(lib().mi_matrix_peer_halo_status(self.h, C.byref(on), C.byref(st)))
        return bool(on.value), int(st.value)

    def dpcg_comm_begin(self, reduce: "Comm", halo: "Comm", patch_rank, patch_nbr_patch=None, n_global=0):
        pr = np.ascontiguousarray(patch_rank, dtype=np.int32)
        pn = None if patch_nbr_patch is None else np.ascontiguousarray(patch_nbr_patch, dtype=np.int32)
        I32 = C.POINTER(C.c_int32)
        _chk(lib().mi_dpcg_comm_begin(self.h, reduce.h, halo.h, pr.ctypes.data_as(I32) if pr.size else I32(),
                                      pn.ctypes.data_as(I32) if pn is not None and pn.size else I32(), C.c_int64(n_global)))

    def dpcg_comm_iterate(self, n_iters: int, event_stride: int = 0):
        _chk(lib().mi_dpcg_comm_iterate(self.h, C.c_int32(n_iters), C.c_int32(event_stride)))

    def event_record(self, idx: int):
        _chk(lib().mi_event_record(self.h, C.c_int32(idx)))

    def event_elapsed_ms(self, i0: int, i1: int) -> float:
        ms = C.c_float()
        _chk(lib().mi_event_elapsed_ms(self.h, C.c_int32(i0), C.c_int32(i1), C.byref(ms)))
        return ms.value

    def occupancy(self):
        b, l, s = C.c_int32(), C.c_int32(), C.c_int32()
        _chk(lib().mi_debug_occupancy(self.h, C.byref(b), C.byref(l), C.byref(s)))
        return dict(blocks_per_cu=b.value, lds_bytes=l.value, block_size=s.value)

    def bench_amul(self, reps: int) -> float:
        ms = C.c_float()
        _chk(lib().mi_bench_amul(self.h, C.c_int32(reps), C.byref(ms)))
        return ms.value

    def close(self):
        if self.h:
            lib().mi_matrix_destroy(self.h)
            self.h = C.c_void_p()


class Gamg:
    """GAMG hierarchy + solver (lduMatrix::solver 'GAMG', agglomerator faceAreaPair/algebraicPair)."""

    def __init__(self, addr: Addressing, face_weights, n_cells_in_coarsest_level: int = 10, forward: bool = True,
                 comms=None, patch_rank=None, patch_nbr_patch=None, merge_levels: int = 1, dummy_levels: int = 0):
        """comms = (reduce, halo) Comm pair of a decomposed case (the matrix must be attached to the same pair);
        dummy_levels n > 0: the reference's dummyAgglomeration (n identity levels), face_weights unused"""
        self.addr = addr
        self.h = C.c_void_p()
        if dummy_levels > 0:
            _chk(lib().mi_gamg_create_dummy(addr.h, C.c_int32(dummy_levels), C.byref(self.h)))
            self._keep = None
            self.n_levels = int(lib().mi_gamg_n_levels(self.h))
            self.forward_out = bool(lib().mi_gamg_forward_out(self.h))
            return
        w = np.ascontiguousarray(face_weights, dtype=np.float64)
        I32 = C.POINTER(C.c_int32)
        pr = None if patch_rank is None else np.ascontiguousarray(patch_rank, dtype=np.int32)
        pn = None if patch_nbr_patch is None else np.ascontiguousarray(patch_nbr_patch, dtype=np.int32)
        _chk(lib().mi_gamg_create_coupled(addr.h, w.ctypes.data_as(C.POINTER(C.c_double)), C.c_int32(n_cells_in_coarsest_level),
                                          C.c_int32(merge_levels), int(forward), comms[0].h if comms else C.c_void_p(), comms[1].h if comms else C.c_void_p(),
                                          pr.ctypes.data_as(I32) if pr is not None and pr.size else I32(),
                                          pn.ctypes.data_as(I32) if pn is not None and pn.size else I32(), C.byref(self.h)))
        self._keep = (comms, pr, pn)
        self.n_levels = int(lib().mi_gamg_n_levels(self.h))
        self.forward_out = bool(lib().mi_gamg_forward_out(self.h))

    def level_sizes(self, level: int):
        out = (C.c_int32 * 4)()
        _chk(lib().mi_gamg_level_sizes(self.h, C.c_int32(level), out))
        return dict(zip(("n_fine", "n_fine_faces", "n_coarse", "n_coarse_faces"), [int(v) for v in out]))

    def solve(self, mat: Matrix, psi, source, **kw):
        ctl = gamg_controls(**kw)
        perf = SolverPerf()
        hist_len = ctl.maxIter + 2
        hist = np.full(hist_len, np.nan)
        _chk(lib().mi_gamg_solve(self.h, mat.h, _ptr(psi), _ptr(source), C.byref(ctl), C.byref(perf),
                                 hist.ctypes.data_as(C.POINTER(C.c_double)), C.c_int32(hist_len)))
        out = {k: getattr(perf, k) for k, _ in SolverPerf._fields_ if k != "reserved"}
        out["history"] = hist[~np.isnan(hist)].copy()
        return out

    def restrict(self, level, fine, coarse):
        _chk(lib().mi_gamg_restrict(self.h, C.c_int32(level), _ptr(fine), _ptr(coarse)))

    def prolong(self, level, coarse, fine):
        _chk(lib().mi_gamg_prolong(self.h, C.c_int32(level), _ptr(coarse), _ptr(fine)))

    def level_coeffs(self, mat: Matrix, level, diag, upper, lower=None):
        _chk(lib().mi_gamg_level_coeffs(self.h, mat.h, C.c_int32(level), _ptr(diag), _ptr(upper), _ptr(lower)))

    def close(self):
        if self.h:
            lib().mi_gamg_destroy(self.h)
            self.h = C.c_void_p()


def gamg_host_hierarchy_domains(domains, face_weights_per_domain, n_cells_in_coarsest_level=10, forward=True, merge_levels=1):
    """Host-only build of the per-rank GAMG hierarchies of a decomposed case (list of LduCase sub-domains with interfaces), all
    domains in this process; returns [domain][level] dicts incl. "patches": [{faceRestrict, faceCells, nbrCells}] (tests)."""
    I32P, F64P = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    D = len(domains)
    keep = []
    def i32(a):
        a = np.ascontiguousarray(a, dtype=np.int32); keep.append(a); return a.ctypes.data_as(I32P)
    n_cells = (C.c_int32 * D)(*[d.n_cells for d in domains]); n_faces = (C.c_int32 * D)(*[d.n_faces for d in domains])
    lower = (I32P * D)(*[i32(d.lower_addr) for d in domains]); upper = (I32P * D)(*[i32(d.upper_addr) for d in domains])
    ws = [np.ascontiguousarray(w, dtype=np.float64) for w in face_weights_per_domain]; keep.append(ws)
    weights = (F64P * D)(*[w.ctypes.data_as(F64P) for w in ws])
    n_patches = (C.c_int32 * D)(*[len(d.interfaces) for d in domains])
    sizes = (I32P * D)(*[i32([len(i.face_cells) for i in d.interfaces] or [0]) for d in domains])
    nbr_d = (I32P * D)(*[i32([i.nbr_domain for i in d.interfaces] or [0]) for d in domains])
    nbr_p = (I32P * D)(*[i32([i.nbr_patch for i in d.interfaces] or [0]) for d in domains])
    fcs = []
    for d in domains:
        arr = (I32P * max(len(d.interfaces), 1))(*[i32(i.face_cells) for i in d.interfaces]); keep.append(arr); fcs.append(arr)
    PP = C.POINTER(I32P)
    fc = (PP * D)(*[C.cast(a, PP) for a in fcs])
    out = (C.c_void_p * D)()
    _chk(lib().mi_gamg_host_build_domains(C.c_int32(D), n_cells, n_faces, lower, upper, weights, n_patches, sizes, fc, nbr_d, nbr_p,
                                          C.c_int32(n_cells_in_coarsest_level), C.c_int32(merge_levels), int(forward), out))
    res = []
    try:
        for d in range(D):
            h = C.c_void_p(out[d]); levels = []
            for lvl in range(int(lib().mi_gamg_host_n_levels(h))):
                lv = {}
                for name in ("restrictMap", "faceRestrict", "cLower", "cUpper"):
                    data, ln, es = C.c_void_p(), C.c_int64(), C.c_int32()
                    _chk(lib().mi_gamg_host_array(h, C.c_int32(lvl), name.encode(), C.byref(data), C.byref(ln), C.byref(es)))
                    lv[name] = np.frombuffer((C.c_char * (ln.value * 4)).from_address(data.value), dtype=np.int32).copy() if ln.value else np.zeros(0, np.int32)
                lv["patches"] = []
                for p in range(len(domains[d].interfaces)):
                    pd = {}
                    for name in ("faceRestrict", "faceCells", "nbrCells"):
                        data, ln = C.c_void_p(), C.c_int64()
                        _chk(lib().mi_gamg_host_patch_array(h, C.c_int32(lvl), C.c_int32(p), name.encode(), C.byref(data), C.byref(ln)))
                        pd[name] = np.frombuffer((C.c_char * (ln.value * 4)).from_address(data.value), dtype=np.int32).copy() if ln.value else np.zeros(0, np.int32)
                    lv["patches"].append(pd)
                levels.append(lv)
            res.append(levels)
    finally:
        for d in range(D):
            lib().mi_gamg_host_free(C.c_void_p(out[d]))
    return res


def gamg_host_hierarchy_ami(case, face_weights, n_cells_in_coarsest_level=10):
    """Host-only build of the GAMG hierarchy of ONE domain whose interfaces are all cyclicAMI (LduCase with ami_* fields);
    returns [level] dicts incl. "patches": [{faceRestrict, faceCells, amiStart, amiAddr, amiW, amiMagSf}] (CPU tests)."""
    I32P, F64P = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    keep = []
    def i32(a):
        a = np.ascontiguousarray(a, dtype=np.int32); keep.append(a); return a.ctypes.data_as(I32P)
    def f64(a):
        a = np.ascontiguousarray(a, dtype=np.float64); keep.append(a); return a.ctypes.data_as(F64P)
    P = len(case.interfaces)
    sizes = i32([len(i.face_cells) for i in case.interfaces]); nbr = i32([i.nbr_patch for i in case.interfaces])
    fc = (I32P * P)(*[i32(i.face_cells) for i in case.interfaces])
    st = (I32P * P)(*[i32(i.ami_start) for i in case.interfaces]); ad = (I32P * P)(*[i32(i.ami_addr) for i in case.interfaces])
    ww = (F64P * P)(*[f64(i.ami_w) for i in case.interfaces]); ms = (F64P * P)(*[f64(i.ami_magsf) for i in case.interfaces])
    h = C.c_void_p()
    _chk(lib().mi_gamg_host_build_ami(C.c_int32(case.n_cells), C.c_int32(case.n_faces), i32(case.lower_addr), i32(case.upper_addr), f64(face_weights),
                                      C.c_int32(n_cells_in_coarsest_level), C.c_int32(P), sizes, fc, nbr, st, ad, ww, ms, C.byref(h)))
    levels = []
    try:
        for lvl in range(int(lib().mi_gamg_host_n_levels(h))):
            lv = {}
            for name in ("restrictMap",):
                data, ln, es = C.c_void_p(), C.c_int64(), C.c_int32()
                _chk(lib().mi_gamg_host_array(h, C.c_int32(lvl), name.encode(), C.byref(data), C.byref(ln), C.byref(es)))
                lv[name] = np.frombuffer((C.c_char * (ln.value * 4)).from_address(data.value), dtype=np.int32).copy()
            lv["patches"] = []
            for p in range(P):
                pd = {}
                for name, dt in (("faceRestrict", np.int32), ("faceCells", np.int32), ("amiStart", np.int32), ("amiAddr", np.int32), ("amiW", np.float64), ("amiMagSf", np.float64)):
                    data, ln = C.c_void_p(), C.c_int64()
                    _chk(lib().mi_gamg_host_patch_array(h, C.c_int32(lvl), C.c_int32(p), name.encode(), C.byref(data), C.byref(ln)))
                    nb = ln.value * np.dtype(dt).itemsize
                    pd[name] = np.frombuffer((C.c_char * nb).from_address(data.value), dtype=dt).copy() if ln.value else np.zeros(0, dt)
                lv["patches"].append(pd)
            levels.append(lv)
    finally:
        lib().mi_gamg_host_free(h)
    return levels


def gamg_host_hierarchy(n_cells, lower_addr, upper_addr, face_weights, n_cells_in_coarsest_level=10, forward=True, merge_levels=1):
    """Host-only build of the GAMG hierarchy; returns a list of per-level dicts of numpy arrays (tests)."""
    lo = np.ascontiguousarray(lower_addr, dtype=np.int32)
    up = np.ascontiguousarray(upper_addr, dtype=np.int32)
    w = np.ascontiguousarray(face_weights, dtype=np.float64)
    h = C.c_void_p()
    _chk(lib().mi_gamg_host_build(C.c_int32(n_cells), C.c_int32(lo.shape[0]), lo.ctypes.data_as(C.POINTER(C.c_int32)),
                                  up.ctypes.data_as(C.POINTER(C.c_int32)), w.ctypes.data_as(C.POINTER(C.c_double)),
                                  C.c_int32(n_cells_in_coarsest_level), C.c_int32(merge_levels), int(forward), C.byref(h)))
    out = []
    try:
        for lvl in range(int(lib().mi_gamg_host_n_levels(h))):
            d = {}
            for name in ("restrictMap", "faceRestrict", "faceFlip", "cLower", "cUpper", "cellChildStart", "cellChild",
                         "faceChildStart", "faceChild", "diagChildStart", "diagChild"):
                data, ln, es = C.c_void_p(), C.c_int64(), C.c_int32()
                _chk(lib().mi_gamg_host_array(h, C.c_int32(lvl), name.encode(), C.byref(data), C.byref(ln), C.byref(es)))
                dt = np.uint8 if es.value == 1 else np.int32
                if ln.value:
                    buf = (C.c_char * (ln.value * es.value)).from_address(data.value)
                    d[name] = np.frombuffer(buf, dtype=dt).copy()
                else:
                    d[name] = np.zeros(0, dtype=dt)
            out.append(d)
    finally:
        lib().mi_gamg_host_free(h)
    return out


class PatchNhatf(C.Structure):
    """mi_patch_nhatf (include/mi_ldu.h)"""
    _fields_ = [("patch_weights_dev", C.c_void_p), ("grad_dev", C.c_void_p * 3), ("nbr_grad_dev", C.c_void_p * 3), ("patch_sf_dev", C.c_void_p * 3),
                ("patch_magsf_dev", C.c_void_p), ("theta_deg_dev", C.c_void_p), ("nhatf_out_dev", C.c_void_p), ("nhatfv_out_dev", C.c_void_p * 3),
                ("gradient_out_dev", C.c_void_p), ("b1_out_dev", C.c_void_p), ("b2_out_dev", C.c_void_p)]


class Patch:
    """A boundary patch (its faceCells) for the assembly sweeps."""

    def __init__(self, ctx: Context, n_cells: int, face_cells):
        fc = np.ascontiguousarray(face_cells, dtype=np.int32)
        self.h = C.c_void_p()
        _chk(lib().mi_patch_create(ctx.h, C.c_int32(n_cells), C.c_int32(fc.shape[0]),
                                   fc.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(self.h)))

    def add(self, pf, intf, fn: int = 0):
        _chk(lib().mi_patch_add(self.h, _ptr(pf), _ptr(intf), int(fn)))

    def max(self, pf, cell_inout):
        """cell_inout[faceCells] = max(cell_inout[faceCells], pf): the patch part of CoEuler's CorDeltaT (mi_patch_max)"""
        _chk(lib().mi_patch_max(self.h, _ptr(pf), _ptr(cell_inout)))

    def add_product(self, pf, q, intf, fn: int = 0):
        """intf[faceCells] += pf*q (coupled part of addBoundarySource)"""
        _chk(lib().mi_patch_add_product(self.h, _ptr(pf), _ptr(q), _ptr(intf), int(fn)))

    def flux(self, internal_coeffs, boundary_coeffs, psi, out, patch_neighbour_field=None):
        """boundary part of fvMatrix::flux; patch_neighbour_field only for coupled patches"""
        _chk(lib().mi_patch_flux(self.h, _ptr(internal_coeffs), _ptr(boundary_coeffs), _ptr(psi), _ptr(patch_neighbour_field), _ptr(out)))

    def internal_field(self, psi, out):
        """fvPatchField::patchInternalField: out[i] = psi[faceCells[i]]"""
        _chk(lib().mi_patch_internal_field(self.h, _ptr(psi), _ptr(out)))

    def linear_upwind_correction(self, patch_flux, patch_cf, c, patch_delta, grad, nbr_grad, out, scale=1.0):
        """patchFlux*correction(vf) of linearUpwind (scale 1) / LUST (scale 0.25) on a COUPLED patch (linearUpwind.C:49-62): grad and nbr_grad one
        [gx, gy, gz] per component (cell gradients / their patchNeighbourField), out one patch array per component"""
        n = len(out)
        _chk(lib().mi_patch_linear_upwind_correction(self.h, C.c_double(scale), C.c_int32(n), _ptr(patch_flux), _ptrs(patch_cf), _ptrs(c), _ptrs(patch_delta),
                                                     _ptrs([g for gr in grad for g in gr]), _ptrs([g for gr in nbr_grad for g in gr]), _ptrs(out)))

    def limited_weights(self, lim, patch_cd_weights, patch_flux, phi, nbr_phi, grad, nbr_grad, patch_delta, w_out, limiter_out=None):
        """a limited scheme's weights on a COUPLED patch (LimitedScheme.C:145-195): phi / nbr_phi 1 or 3 arrays (cell field, its
        patchNeighbourField), grad / nbr_grad 3 or 9 (grad[3*j + k] = d(phi_j)/dx_k), patch_delta [x, y, z]; lim a Limiter or a scheme name"""
        lim = limiter(lim) if isinstance(lim, str) else lim
        _chk(lib().mi_patch_limited_weights(self.h, C.byref(lim), _ptr(patch_cd_weights), _ptr(patch_flux), _ptrs(phi), _ptrs(nbr_phi), _ptrs(grad),
                                            _ptrs(nbr_grad), _ptrs(patch_delta), _ptr(w_out), _ptr(limiter_out)))

    def filtered_weights(self, lim, patch_cd_weights, patch_flux, phi, nbr_phi, grad, nbr_grad, patch_delta, w_out, limiter_out=None):
        """a filtered scheme's weights on a COUPLED patch (mi_patch_filtered_weights): the arguments of limited_weights; lim a FilteredLimiter
        or a scheme name"""
        lim = filtered(lim) if isinstance(lim, str) else lim
        _chk(lib().mi_patch_filtered_weights(self.h, C.byref(lim), _ptr(patch_cd_weights), _ptr(patch_flux), _ptrs(phi), _ptrs(nbr_phi), _ptrs(grad),
                                             _ptrs(nbr_grad), _ptrs(patch_delta), _ptr(w_out), _ptr(limiter_out)))

    def interface_compression_weights(self, patch_cd_weights, patch_flux, alpha, nbr_alpha, w_out, limiter_out=None):
        """the interfaceCompression scheme's weights on a COUPLED patch (PhiScheme.C:145-189): alpha the cell field, nbr_alpha its
        patchNeighbourField"""
        _chk(lib().mi_patch_interface_compression_weights(self.h, _ptr(patch_cd_weights), _ptr(patch_flux), _ptr(alpha), _ptr(nbr_alpha), _ptr(w_out),
                                                          _ptr(limiter_out)))

    def alpha_compression_flux(self, patch_cd_weights, patch_phir, alpha1, nbr_alpha1, out):
        """alphaEqn.H's compression flux on a COUPLED patch (mi_patch_alpha_compression_flux)"""
        _chk(lib().mi_patch_alpha_compression_flux(self.h, _ptr(patch_cd_weights), _ptr(patch_phir), _ptr(alpha1), _ptr(nbr_alpha1), _ptr(out)))

    def interface_nhatf(self, delta_n, grad, patch_sf, nhatf_out, patch_weights=None, nbr_grad=None, nhatfv_out=None, patch_magsf=None,
                        theta_deg=None, gradient_out=None, b12_out=None):
        """nHatf on this patch (mi_patch_interface_nhatf).  patch_weights given: a COUPLED patch, grad the cell gradient [gx, gy, gz], nbr_grad
        its patchNeighbourField.  patch_weights None: grad the boundary value of gradAlpha per patch face.  theta_deg given (with patch_magsf):
        a contact-angle patch, correctContactAngle between the unit normal and the flux; gradient_out the gradient of the alphaContactAngle
        patch field, b12_out = (b1, b2) the device's own cos(theta) and cos(acos(a12) - theta)"""
        x = PatchNhatf()
        x.patch_weights_dev = _ptr(patch_weights)
        vec3 = lambda xs: (C.c_void_p * 3)(*[_ptr(v) for v in (xs if xs is not None else (None, None, None))])
        x.grad_dev, x.nbr_grad_dev, x.patch_sf_dev, x.nhatfv_out_dev = vec3(grad), vec3(nbr_grad), vec3(patch_sf), vec3(nhatfv_out)
        x.patch_magsf_dev, x.theta_deg_dev, x.nhatf_out_dev, x.gradient_out_dev = _ptr(patch_magsf), _ptr(theta_deg), _ptr(nhatf_out), _ptr(gradient_out)
        x.b1_out_dev, x.b2_out_dev = (_ptr(b12_out[0]), _ptr(b12_out[1])) if b12_out is not None else (None, None)
        _chk(lib().mi_patch_interface_nhatf(self.h, C.c_double(delta_n), C.byref(x)))

    def central_flux(self, scheme, patch_sf, patch_mag_sf, values, out, patch_weights=None, nbr=None, patch_delta=None):
        """rhoCentralFoam's fluxes on this patch (mi_patch_central_flux).  patch_weights None: values a CentralCells of the seven boundary value
        arrays.  patch_weights given: a COUPLED patch, values the cell arrays, nbr their patchNeighbourFields, patch_delta [x, y, z]"""
        _chk(lib().mi_patch_central_flux(self.h, C.byref(scheme) if scheme is not None else None, _ptr(patch_weights), _ptrs(patch_sf, 3), _ptr(patch_mag_sf),
                                         C.byref(values) if values is not None else None, C.byref(nbr) if nbr is not None else None,
                                         _ptrs(patch_delta, 3), C.byref(out) if out is not None else None))

    def surface_tension_force(self, sigma, patch_weights, patch_delta_coeffs, K, nbr_K, alpha, nbr_alpha, out, sngrad_corr=None):
        """interpolate(sigma*K)*snGrad(alpha) on a COUPLED patch (mi_patch_surface_tension_force): K / alpha the cell fields, nbr_* their
        patchNeighbourFields"""
        _chk(lib().mi_patch_surface_tension_force(self.h, C.c_double(sigma), _ptr(patch_weights), _ptr(patch_delta_coeffs), _ptr(K), _ptr(nbr_K), _ptr(alpha),
                                                  _ptr(nbr_alpha), _ptr(sngrad_corr), _ptr(out)))

    def cubic_correction(self, geo, vf, nbr_vf, grad, nbr_grad, out, patch_flux=None):
        """[patchFlux *] correction(vf) of cubic on a COUPLED patch (mi_patch_cubic_correction): geo a CubicGeometry of the patch's arrays, vf /
        nbr_vf one array per component (cell field, its patchNeighbourField), grad / nbr_grad one [gx, gy, gz] per component, out one patch
        array per component"""
        _chk(lib().mi_patch_cubic_correction(self.h, C.byref(geo), C.c_int32(len(out)), _ptrs(vf), _ptrs(nbr_vf), _ptrs([g for gr in grad for g in gr]),
                                             _ptrs([g for gr in nbr_grad for g in gr]), _ptr(patch_flux), _ptrs(out)))

    def sngrad_correction_flux(self, corr_vecs, weights, grad, nbr_grad, gamma_magsf, out):
        """non-orthogonal correction flux on a COUPLED patch (gaussLaplacianSchemes.C:64-90 + surfaceInterpolationScheme.C:360-365)"""
        _chk(lib().mi_patch_sngrad_correction_flux(self.h, _ptr(corr_vecs[0]), _ptr(corr_vecs[1]), _ptr(corr_vecs[2]), _ptr(weights), _ptr(grad[0]),
                                                   _ptr(grad[1]), _ptr(grad[2]), _ptr(nbr_grad[0]), _ptr(nbr_grad[1]), _ptr(nbr_grad[2]),
                                                   _ptr(gamma_magsf), _ptr(out)))

    def sngrad_limited_correction_flux(self, limit_coeff, corr_vecs, weights, delta_coeffs, vf, nbr_vf, grad, nbr_grad, gamma_magsf, out, limiter_out=None):
        """the `limited` snGrad scheme's correction flux on a COUPLED patch (limitedSnGrad.C:58-84): vf / nbr_vf 1 or 3 arrays (cell field, its
        patchNeighbourField), grad / nbr_grad 3 or 9 (grad[3*j + d] = d(vf_j)/dx_d), out one patch array per component"""
        _chk(lib().mi_patch_sngrad_limited_correction_flux(self.h, C.c_int32(len(vf)), C.c_double(limit_coeff), _ptr(corr_vecs[0]), _ptr(corr_vecs[1]),
                                                           _ptr(corr_vecs[2]), _ptr(weights), _ptr(delta_coeffs), _ptrs(vf), _ptrs(nbr_vf), _ptrs(grad), _ptrs(nbr_grad),
                                                           _ptr(gamma_magsf), _ptrs(out), _ptr(limiter_out)))

    def gauss_grad_correct(self, sf, magsf, sngrad, grad, out):
        """the boundary values of a Gauss gradient on a patch that is NOT coupled (gaussGrad.C:277-303; mi_patch_gauss_grad_correct): sf [x, y, z]
        and magsf patch arrays, sngrad 1 or 3 patch arrays (the field's snGrad on the patch: zeros for zeroGradient), grad 3 or 9 CELL arrays
        (grad[3*j + k] = d(vf_j)/dx_k), out 3 or 9 patch arrays"""
        _chk(lib().mi_patch_gauss_grad_correct(self.h, C.c_int32(len(sngrad)), _ptr(sf[0]), _ptr(sf[1]), _ptr(sf[2]), _ptr(magsf), _ptrs(sngrad), _ptrs(grad), _ptrs(out)))

    def dev_tgrad_flux(self, kind, sf, visc, grad, out, weights=None, nbr_visc=None, nbr_grad=None):
        """Sf_b & (visc*dev[2](T(grad))) on the patch's faces, three components (mi_patch_dev_tgrad_flux); kind "dev" | "dev2".  weights None -- a patch
        that is not coupled: visc and grad[9] are the patch's own boundary values (patch arrays).  weights given -- a coupled patch without
        rotation: visc and grad[9] are the CELL arrays, nbr_visc / nbr_grad[9] their patchNeighbourFields"""
        _chk(lib().mi_patch_dev_tgrad_flux(self.h, C.c_int32(_dev_kind(kind)), _ptr(sf[0]), _ptr(sf[1]), _ptr(sf[2]), _ptr(weights), _ptr(visc), _ptrs(grad),
                                           _ptr(nbr_visc), _ptrs(nbr_grad), _ptrs(out)))

    def close(self):
        if self.h:
            lib().mi_patch_destroy(self.h)
            self.h = C.c_void_p()


class FvmTerms(C.Structure):
    """mi_fvm_terms (include/mi_ldu.h)"""
    _fields_ = [("ddt", C.c_int32), ("r_delta_t", C.c_double), ("rho_value", C.c_double), ("rho_dev", C.c_void_p), ("rho_old_dev", C.c_void_p),
                ("vol_dev", C.c_void_p), ("div_flux_dev", C.c_void_p), ("div_weights_dev", C.c_void_p), ("lap_delta_coeffs_dev", C.c_void_p),
                ("lap_gamma_magsf_dev", C.c_void_p), ("sp_dev", C.c_void_p), ("sp_sign", C.c_double), ("n_rhs", C.c_int32),
                ("psi_old_dev", C.POINTER(C.c_void_p)), ("n_su", C.c_int32), ("su_dev", C.POINTER(C.c_void_p)), ("su_sign", C.POINTER(C.c_double))]


class DdtBackward(C.Structure):
    """mi_ddt_backward (include/mi_ldu.h)"""
    _fields_ = [("coefft", C.c_double), ("coefft0", C.c_double), ("coefft00", C.c_double), ("rho_old_old_dev", C.c_void_p),
                ("psi_old_old_dev", C.POINTER(C.c_void_p))]


def ddt_backward_coeffs(delta_t, delta_t0=None):
    """(coefft, coefft0, coefft00) of the backward scheme (mi_ddt_backward_coeffs; host only, no GPU); delta_t0 None: the first step (the
    field has no old-old time yet, deltaT0 = GREAT)"""
    out = (C.c_double * 3)()
    _chk(lib().mi_ddt_backward_coeffs(C.c_double(delta_t), C.c_double(0.0 if delta_t0 is None else delta_t0), C.c_int32(1 if delta_t0 is None else 2), out))
    return (out[0], out[1], out[2])


class DdtCnState(C.Structure):
    """mi_ddt_cn_state (include/mi_ldu.h)"""
    _fields_ = [("oc", C.c_double), ("start_time_index", C.c_int32), ("ddt0_time_index", C.c_int32)]


class DdtCnScalars(C.Structure):
    """mi_ddt_cn_scalars (include/mi_ldu.h)"""
    _fields_ = [("r_dt_coef", C.c_double), ("r_dt_coef0", C.c_double), ("evaluate", C.c_int32)]


class DdtCnTerms(C.Structure):
    """mi_ddt_cn_terms (include/mi_ldu.h)"""
    _fields_ = [("oc", C.c_double), ("ddt0_dev", C.POINTER(C.c_void_p))]


def ddt_cn_parse(scheme):
    """the off-centring coefficient of `CrankNicolson <oc>` (mi_ddt_cn_parse; host only, no GPU); anything else raises MiError"""
    oc = C.c_double()
    _chk(lib().mi_ddt_cn_parse(str(scheme).encode(), C.byref(oc)))
    return oc.value


class CrankNicolson:
    """The state of one ddt0 field (mi_ddt_cn_state; host only, no GPU): created at `time_index` -- the caller zeroes the ddt0 arrays then.
    step(time_index, delta_t, delta_t0) -> (r_dt_coef, r_dt_coef0, evaluate); evaluate True (once per time step): run Assembly.ddt_cn_update
    with r_dt_coef0 before any other use of ddt0 in this step."""

    def __init__(self, oc, time_index):
        self.state = DdtCnState()
        _chk(lib().mi_ddt_cn_begin(C.c_double(oc), C.c_int32(time_index), C.byref(self.state)))

    @property
    def oc(self):
        return self.state.oc

    def step(self, time_index, delta_t, delta_t0):
        out = DdtCnScalars()
        _chk(lib().mi_ddt_cn_step(C.byref(self.state), C.c_int32(time_index), C.c_double(delta_t), C.c_double(delta_t0), C.byref(out)))
        return (out.r_dt_coef, out.r_dt_coef0, bool(out.evaluate))


class DdtLocalScheme(C.Structure):
    """mi_ddt_local_scheme (include/mi_ldu.h)"""
    _fields_ = [("kind", C.c_int32), ("name", C.c_char * 64), ("rho_name", C.c_char * 64), ("max_co", C.c_double)]


class FvmLocalTerms(C.Structure):
    """mi_fvm_local_terms (include/mi_ldu.h)"""
    _fields_ = [("r_delta_t_dev", C.c_void_p), ("div_flux_dev", C.c_void_p)]


def ddt_local_parse(scheme):
    """`steadyState` -> dict(kind="steadyState"); `localEuler <rDeltaT>` -> dict(kind="localEuler", r_delta_t=name); `CoEuler <phi> <rho> <maxCo>`
    -> dict(kind="CoEuler", phi=, rho=, max_co=) (mi_ddt_local_parse; host only, no GPU); anything else raises MiError"""
    s = DdtLocalScheme()
    _chk(lib().mi_ddt_local_parse(None if scheme is None else str(scheme).encode(), C.byref(s)))
    if s.kind == 0:
        return dict(kind="steadyState")
    if s.kind == 1:
        return dict(kind="localEuler", r_delta_t=s.name.decode())
    return dict(kind="CoEuler", phi=s.name.decode(), rho=s.rho_name.decode(), max_co=s.max_co)


class DivCorrection(C.Structure):
    """mi_div_correction (include/mi_ldu.h)"""
    _fields_ = [("scale", C.c_double), ("cf_dev", C.c_void_p * 3), ("c_dev", C.c_void_p * 3), ("grad_dev", C.c_void_p * 12)]


def div_correction(cf, c, grad, scale=1.0) -> DivCorrection:
    """linearUpwind (scale 1) / LUST (scale 0.25) correction inputs: face centres cf and cell centres c as [x, y, z], grad one [gx, gy, gz]
    per component"""
    k = DivCorrection()
    k.scale = float(scale)
    if len(grad) > 4:
        raise MiError("at most 4 components")
    for d in range(3):
        k.cf_dev[d] = _ptr(cf[d]).value; k.c_dev[d] = _ptr(c[d]).value
    for r, g in enumerate(grad):
        for d in range(3):
            k.grad_dev[3 * r + d] = _ptr(g[d]).value
    return k


class Limiter(C.Structure):
    """mi_limiter (include/mi_ldu.h)"""
    _fields_ = [("kind", C.c_int32), ("vector_form", C.c_int32), ("bounded", C.c_int32), ("k", C.c_double), ("lower", C.c_double), ("upper", C.c_double)]


LIMITER_KINDS = ("limitedLinear", "vanLeer", "MUSCL", "Minmod", "SuperBee", "UMIST", "vanAlbada", "OSPRE", "QUICK", "limitedCubic", "Gamma", "SFCD")


def limiter(scheme: str) -> Limiter:
    """mi_limiter_parse: "vanLeer", "limitedLinearV 1", "limitedCubic01 0.5", "limitedVanLeer -1 2" ... (host only, no GPU)"""
    out = Limiter()
    _chk(lib().mi_limiter_parse(scheme.encode(), C.byref(out)))
    return out


class CentralScheme(C.Structure):
    """mi_central_scheme (include/mi_ldu.h)"""
    _fields_ = [("flux_scheme", C.c_int32), ("reserved", C.c_int32), ("rho", Limiter), ("U", Limiter), ("T", Limiter)]


class CentralCells(C.Structure):
    """mi_central_cells (include/mi_ldu.h)"""
    _fields_ = [("rho_dev", C.c_void_p), ("rhou_dev", C.c_void_p * 3), ("rpsi_dev", C.c_void_p), ("e_dev", C.c_void_p), ("c_dev", C.c_void_p),
                ("grad_rho_dev", C.c_void_p * 3), ("grad_rhou_dev", C.c_void_p * 9), ("grad_rpsi_dev", C.c_void_p * 3), ("grad_e_dev", C.c_void_p * 3),
                ("grad_c_dev", C.c_void_p * 3), ("lim_u_dev", C.c_void_p), ("grad_lim_u_dev", C.c_void_p * 3)]


class CentralOut(C.Structure):
    """mi_central_out (include/mi_ldu.h)"""
    _fields_ = [("phi_out_dev", C.c_void_p), ("phiup_out_dev", C.c_void_p * 3), ("phiep_out_dev", C.c_void_p), ("amaxsf_out_dev", C.c_void_p),
                ("a_pos_out_dev", C.c_void_p), ("au_out_dev", C.c_void_p * 3)]


def central_scheme(flux_scheme: str, reconstruct_rho: str, reconstruct_U: str, reconstruct_T: str) -> CentralScheme:
    """mi_central_scheme_parse: "Kurganov" | "Tadmor" and the three reconstruct(...) entries of fvSchemes, each a limited scheme as
    limiter() reads it; reconstruct(U) a V form or a scalar form (host only, no GPU)"""
    out = CentralScheme()
    _chk(lib().mi_central_scheme_parse(flux_scheme.encode(), reconstruct_rho.encode(), reconstruct_U.encode(), reconstruct_T.encode(), C.byref(out)))
    return out


def _pvec(xs, n):
    """n device pointers of a list that may be None or hold None"""
    xs = list(xs) if xs is not None else []
    return (C.c_void_p * n)(*[_ptr(x) for x in xs + [None] * (n - len(xs))])


def central_cells(rho=None, rhoU=None, rPsi=None, e=None, c=None, grad_rho=None, grad_rhoU=None, grad_rPsi=None, grad_e=None, grad_c=None,
                  lim_U=None, grad_lim_U=None) -> CentralCells:
    """one side's fields of the central flux passes: cell arrays, patchNeighbourFields or a plain patch's boundary values; rhoU three arrays,
    every gradient three, grad_rhoU nine (grad_rhoU[3*j + k] = d(rhoU_j)/dx_k); lim_U / grad_lim_U for a scalar reconstruct(U).  The
    structure holds device addresses, not tensors: the caller keeps the tensors alive until the call has been made"""
    x = CentralCells()
    x.rho_dev, x.rpsi_dev, x.e_dev, x.c_dev, x.lim_u_dev = _ptr(rho), _ptr(rPsi), _ptr(e), _ptr(c), _ptr(lim_U)
    x.rhou_dev, x.grad_rho_dev, x.grad_rpsi_dev, x.grad_e_dev, x.grad_c_dev = _pvec(rhoU, 3), _pvec(grad_rho, 3), _pvec(grad_rPsi, 3), _pvec(grad_e, 3), _pvec(grad_c, 3)
    x.grad_rhou_dev, x.grad_lim_u_dev = _pvec(grad_rhoU, 9), _pvec(grad_lim_U, 3)
    return x


def central_out(phi=None, phiUp=None, phiEp=None, amaxSf=None, a_pos=None, aU=None) -> CentralOut:
    """the outputs of the central flux passes: phiUp three arrays; a_pos and aU (three arrays) together or not at all"""
    x = CentralOut()
    x.phi_out_dev, x.phiep_out_dev, x.amaxsf_out_dev, x.a_pos_out_dev = _ptr(phi), _ptr(phiEp), _ptr(amaxSf), _ptr(a_pos)
    x.phiup_out_dev, x.au_out_dev = _pvec(phiUp, 3), _pvec(aU, 3)
    return x


class FilteredLimiter(C.Structure):
    """mi_filtered_limiter (include/mi_ldu.h)"""
    _fields_ = [("kind", C.c_int32), ("vector_form", C.c_int32), ("k", C.c_double), ("l", C.c_double)]


FILTERED_KINDS = ("filteredLinear", "filteredLinear2", "filteredLinear3")


def filtered(scheme: str) -> FilteredLimiter:
    """mi_filtered_parse: "filteredLinear", "filteredLinear2 1 0", "filteredLinear2V 1 0", "filteredLinear3 0.5", "filteredLinear3V 0.5" (host only,
    no GPU); l stays as written (the engine adds the constructor's 1.0)"""
    out = FilteredLimiter()
    _chk(lib().mi_filtered_parse(scheme.encode(), C.byref(out)))
    return out


def interface_compression(scheme: str) -> None:
    """mi_interface_compression_parse: raises unless the scheme is exactly "interfaceCompression" (host only, no GPU)"""
    _chk(lib().mi_interface_compression_parse(scheme.encode()))


class CubicGeometry(C.Structure):
    """mi_cubic_geometry (include/mi_ldu.h)"""
    _fields_ = [("lambda_dev", C.c_void_p), ("sf_dev", C.c_void_p * 3), ("mag_sf_dev", C.c_void_p), ("delta_coeffs_dev", C.c_void_p)]


def cubic_geometry(lam, sf, mag_sf, delta_coeffs) -> CubicGeometry:
    """the face geometry the cubic correction reads: mesh.weights(), Sf as [x, y, z], magSf, surfaceInterpolation::deltaCoeffs() (of the
    internal faces, or of one coupled patch)"""
    g = CubicGeometry()
    g.lambda_dev = _ptr(lam).value; g.mag_sf_dev = _ptr(mag_sf).value; g.delta_coeffs_dev = _ptr(delta_coeffs).value
    for d in range(3):
        g.sf_dev[d] = _ptr(sf[d]).value
    g.arrays = (lam, tuple(sf), mag_sf, delta_coeffs)   # the struct holds bare addresses: keep the tensors alive as long as it lives
    return g


class GradLimiter(C.Structure):
    """mi_grad_limiter (include/mi_ldu.h)"""
    _fields_ = [("kind", C.c_int32), ("identity", C.c_int32), ("k", C.c_double)]


GRAD_LIMITER_KINDS = ("cellLimited", "cellMDLimited", "faceLimited", "faceMDLimited")
GRAD_PATCH_KINDS = {"other": 0, "coupled": 1, "fixesValue": 2}


def grad_limiter(scheme: str) -> GradLimiter:
    """mi_grad_limiter_parse: "cellLimited Gauss linear 1", "faceMDLimited Gauss linear 0.5" ... (host only, no GPU)"""
    out = GradLimiter()
    _chk(lib().mi_grad_limiter_parse(scheme.encode(), C.byref(out)))
    return out


class SnGradScheme(C.Structure):
    """mi_sngrad_scheme (include/mi_ldu.h)"""
    _fields_ = [("kind", C.c_int32), ("limit_coeff", C.c_double)]


SNGRAD_KINDS = ("uncorrected", "orthogonal", "corrected", "limited")


def sngrad_parse(text: str) -> SnGradScheme:
    """mi_sngrad_parse: "uncorrected", "orthogonal", "corrected", "limited 0.5", "limited corrected 0.33" (host only, no GPU)"""
    out = SnGradScheme()
    _chk(lib().mi_sngrad_parse(text.encode(), C.byref(out)))
    return out


DEV_KINDS = ("dev", "dev2")        # MI_DEV, MI_DEV2: dev(T(grad(U))) of divDevReff, dev2(T(grad(U))) of divDevRhoReff


def _dev_kind(kind) -> int:
    """"dev" | "dev2" (or the number itself: the library refuses what it does not know)"""
    return DEV_KINDS.index(kind) if kind in DEV_KINDS else int(kind)


class GradBoundary:
    """The boundary of a limited gradient (mi_grad_boundary_create): the patches in order, each its faceCells and a kind ("coupled",
    "fixesValue", "other"); boundary face fields are the patch-ordered concatenation of their faces (n_faces)."""

    def __init__(self, addr: Addressing, face_cells: Sequence, kinds: Sequence):
        fcs = [np.ascontiguousarray(f, dtype=np.int32) for f in face_cells]
        n = len(fcs)
        if len(kinds) != n:
            raise MiError("one kind per patch")
        I32 = C.POINTER(C.c_int32)
        sizes = (C.c_int32 * max(n, 1))(*[f.shape[0] for f in fcs])
        ptrs = (I32 * max(n, 1))(*[f.ctypes.data_as(I32) for f in fcs])
        kd = (C.c_int32 * max(n, 1))(*[GRAD_PATCH_KINDS[k] if isinstance(k, str) else int(k) for k in kinds])
        self.addr = addr
        self.n_faces = int(sum(f.shape[0] for f in fcs))
        self.h = C.c_void_p()
        _chk(lib().mi_grad_boundary_create(addr.h, C.c_int32(n), sizes, ptrs, kd, C.byref(self.h)))

    def close(self):
        if self.h:
            lib().mi_grad_boundary_destroy(self.h)
            self.h = C.c_void_p()


class GradScheme(C.Structure):
    """mi_grad_scheme (include/mi_ldu.h)"""
    _fields_ = [("base", C.c_int32), ("limited", C.c_int32), ("limiter", GradLimiter)]


GRAD_BASES = ("Gauss linear", "leastSquares")


def grad_scheme(scheme: str) -> GradScheme:
    """mi_grad_scheme_parse: a gradSchemes entry -- "Gauss linear", "leastSquares", "cellLimited leastSquares 1",
    "faceMDLimited Gauss linear 0.5" ... (host only, no GPU)"""
    out = GradScheme()
    _chk(lib().mi_grad_scheme_parse(scheme.encode(), C.byref(out)))
    return out


class LsVectors:
    """The least-squares vectors of a mesh, built once on the device (mi_ls_vectors_create): centres [x, y, z] cell arrays, weights / mag_sf
    internal-face arrays, b_weights / b_mag_sf / b_delta ([x, y, z]) boundary-face arrays in the patch order of `boundary` (a GradBoundary or
    None; b_weights is read on coupled patches only).  The boundary must stay open as long as the vectors are used."""

    def __init__(self, addr: Addressing, boundary, centres, weights, mag_sf, b_weights=None, b_mag_sf=None, b_delta=None):
        self.addr, self.boundary = addr, boundary
        self.h = C.c_void_p()
        _chk(lib().mi_ls_vectors_create(addr.h, boundary.h if boundary is not None else None, _ptrs(centres), _ptr(weights), _ptr(mag_sf),
                                        _ptr(b_weights), _ptr(b_mag_sf), _ptrs(b_delta), C.byref(self.h)))

    def fields(self, p_out, n_out, bp_out=None):
        """copies pVectors, nVectors (internal faces) and the boundary pVectors into three arrays each (mi_ls_vectors_fields)"""
        _chk(lib().mi_ls_vectors_fields(self.h, _ptrs(p_out), _ptrs(n_out), _ptrs(bp_out)))

    def close(self):
        if self.h:
            lib().mi_ls_vectors_destroy(self.h)
            self.h = C.c_void_p()


SURFACE_SUM_MODES = ("sum", "mag")


class Reconstruct:
    """fvc::reconstruct's data of a mesh, built once on the device (mi_reconstruct_create): sf [x, y, z] / mag_sf internal-face arrays, b_sf /
    b_mag_sf boundary-face arrays in the patch order of `boundary` (a GradBoundary or None: no boundary faces).  The handle keeps SfHat and
    the inverse geometric tensor; the boundary must stay open as long as it is used.  After mesh motion: close and build again."""

    def __init__(self, addr: Addressing, boundary, sf, mag_sf, b_sf=None, b_mag_sf=None):
        self.addr, self.boundary = addr, boundary
        self.h = C.c_void_p()
        _chk(lib().mi_reconstruct_create(addr.h, boundary.h if boundary is not None else None, _ptrs(sf), _ptr(mag_sf), _ptrs(b_sf), _ptr(b_mag_sf),
                                         C.byref(self.h)))

    def fields(self, inv_out):
        """copies the inverse tensor into nine cell arrays xx xy xz yx yy yz zx zy zz (mi_reconstruct_fields) -> removeCmpts as (x, y, z) of 0 / 1"""
        removed = (C.c_int32 * 3)(0, 0, 0)
        _chk(lib().mi_reconstruct_fields(self.h, _ptrs(inv_out), removed))
        return tuple(int(x) for x in removed)

    def close(self):
        if self.h:
            lib().mi_reconstruct_destroy(self.h)
            self.h = C.c_void_p()


def reconstruct_create(addr: Addressing, boundary, sf, mag_sf, b_sf=None, b_mag_sf=None) -> Reconstruct:
    return Reconstruct(addr, boundary, sf, mag_sf, b_sf, b_mag_sf)


def reconstruct_fields(rc: Reconstruct, inv_out):
    return rc.fields(inv_out)


def reconstruct_destroy(rc: Reconstruct):
    rc.close()


class MulesFields(C.Structure):
    """mi_mules_fields (include/mi_ldu.h)"""
    _fields_ = [("r_delta_t", C.c_double), ("r_delta_t_dev", C.c_void_p), ("rho_dev", C.c_void_p), ("rho_old_dev", C.c_void_p),
                ("sp_dev", C.c_void_p), ("su_dev", C.c_void_p), ("vol_dev", C.c_void_p), ("psi_dev", C.c_void_p), ("psi_old_dev", C.c_void_p),
                ("b_psi_dev", C.c_void_p), ("psi_max", C.c_double), ("psi_min", C.c_double)]


class MulesFlux(C.Structure):
    """mi_mules_flux (include/mi_ldu.h)"""
    _fields_ = [(name, C.c_void_p) for name in ("phi_dev", "b_phi_dev", "phi_psi_dev", "b_phi_psi_dev", "phi_bd_dev", "b_phi_bd_dev", "phi_corr_dev",
                                                "b_phi_corr_dev", "lambda_dev", "b_lambda_dev", "out_dev", "b_out_dev")]


MULES_FORMS = ("limiter", "limit")      # MI_MULES_LIMITER, MI_MULES_LIMIT
MULES_CORR_FORMS = ("limiter", "limit")  # MI_MULES_CORR_LIMITER, MI_MULES_CORR_LIMIT


def mules_fields(vol, psi, psi_old, r_delta_t=1.0, b_psi=None, psi_max=1.0, psi_min=0.0, rho=None, rho_old=None, sp=None, su=None):
    """mi_mules_fields: r_delta_t a number, or a cell tensor (explicitLTSSolve); rho and rho_old both or neither; sp / su or None; b_psi the
    patch-ordered boundary values (patchNeighbourField on coupled patches).  Returns the structure; it keeps the tensors alive"""
    lts = not isinstance(r_delta_t, (int, float))
    f = MulesFields(0.0 if lts else float(r_delta_t), _ptr(r_delta_t) if lts else None, _ptr(rho), _ptr(rho_old), _ptr(sp), _ptr(su), _ptr(vol),
                    _ptr(psi), _ptr(psi_old), _ptr(b_psi), float(psi_max), float(psi_min))
    f._keep = (r_delta_t, rho, rho_old, sp, su, vol, psi, psi_old, b_psi)
    return f


def mules_flux(**arrays):
    """mi_mules_flux from keywords: phi, phi_psi, phi_bd, phi_corr, lambda_, out and their boundary twins b_phi, ... (None: not given)"""
    x = MulesFlux()
    for key, t in arrays.items():
        name = key.rstrip("_") + "_dev"
        if not hasattr(x, name):
            raise MiError("mules_flux: unknown array '%s'" % key)
        setattr(x, name, _ptr(t))
    x._keep = arrays
    return x


class Mules:
    """Explicit MULES on one mesh (mi_mules_create): boundary a GradBoundary or None (no boundary faces), wedge one flag per patch or None.
    The handle owns the six cell work arrays, so no call allocates; the boundary must stay open as long as it is used.  fields is a
    mules_fields(...), flux a mules_flux(...)."""

    def __init__(self, addr: Addressing, boundary=None, wedge=None):
        self.addr, self.boundary = addr, boundary
        self.h = C.c_void_p()
        w = None if wedge is None else (C.c_int32 * max(len(wedge), 1))(*[int(bool(x)) for x in wedge])
        _chk(lib().mi_mules_create(addr.h, boundary.h if boundary is not None else None, w, C.byref(self.h)))

    def work(self, out):
        """copies psiMaxn, psiMinn (transformed), sumPhip, mSumPhim, lambdap, lambdam into six cell arrays (mi_mules_work)"""
        pv = None if out is None else (C.c_void_p * 6)(*[_ptr(x) for x in out])
        _chk(lib().mi_mules_work(self.h, pv))

    def begin(self, form, fields, flux):
        f = MULES_FORMS.index(form) if form in MULES_FORMS else int(form)
        _chk(lib().mi_mules_begin(self.h, C.c_int32(f), C.byref(fields) if fields is not None else None, C.byref(flux) if flux is not None else None))

    def iterate(self, n, fields, flux):
        _chk(lib().mi_mules_iterate(self.h, C.c_int32(n), C.byref(fields) if fields is not None else None, C.byref(flux) if flux is not None else None))

    def apply(self, return_corr, fields, flux):
        _chk(lib().mi_mules_apply(self.h, C.c_int32(int(bool(return_corr))), C.byref(fields) if fields is not None else None,
                                  C.byref(flux) if flux is not None else None))

    def limiter(self, fields, flux, n_limiter_iter=3):
        """MULES::limiter: begin("limiter") + iterate(n_limiter_iter)"""
        _chk(lib().mi_mules_limiter(self.h, C.c_int32(n_limiter_iter), C.byref(fields) if fields is not None else None,
                                    C.byref(flux) if flux is not None else None))

    def limit(self, fields, flux, n_limiter_iter=3, return_corr=False):
        """MULES::limit: begin("limit") + iterate(n_limiter_iter) + apply(return_corr)"""
        _chk(lib().mi_mules_limit(self.h, C.c_int32(n_limiter_iter), C.c_int32(int(bool(return_corr))), C.byref(fields) if fields is not None else None,
                                  C.byref(flux) if flux is not None else None))

    def explicit_solve(self, fields, phi_psi, psi_out, b_phi_psi=None):
        """MULES::explicitSolve(rDeltaT, rho, psi, phiPsi, Sp, Su): the new psi into psi_out"""
        _chk(lib().mi_mules_explicit_solve(self.h, C.byref(fields) if fields is not None else None, _ptr(phi_psi), _ptr(b_phi_psi), _ptr(psi_out)))

    def begin_corr(self, form, fields, flux, extrema_coeff=0.0):
        f = MULES_CORR_FORMS.index(form) if form in MULES_CORR_FORMS else int(form)
        _chk(lib().mi_mules_begin_corr(self.h, C.c_int32(f), C.c_double(extrema_coeff), C.byref(fields) if fields is not None else None,
                                       C.byref(flux) if flux is not None else None))

    def limiter_corr(self, fields, flux, n_limiter_iter=3, extrema_coeff=0.0):
        """MULES::limiterCorr: begin_corr("limiter") + iterate(n_limiter_iter)"""
        _chk(lib().mi_mules_limiter_corr(self.h, C.c_int32(n_limiter_iter), C.c_double(extrema_coeff), C.byref(fields) if fields is not None else None,
                                         C.byref(flux) if flux is not None else None))

    def limit_corr(self, fields, flux, n_limiter_iter=3, extrema_coeff=0.0):
        """MULES::limitCorr: begin_corr("limit") + iterate(n_limiter_iter) + phi_corr *= lambda in place"""
        _chk(lib().mi_mules_limit_corr(self.h, C.c_int32(n_limiter_iter), C.c_double(extrema_coeff), C.byref(fields) if fields is not None else None,
                                       C.byref(flux) if flux is not None else None))

    def correct(self, fields, phi_corr, psi_inout, b_phi_corr=None):
        """MULES::correct(rDeltaT, rho, psi, phi, phiCorr, Sp, Su): psi_inout updated in place"""
        _chk(lib().mi_mules_correct(self.h, C.byref(fields) if fields is not None else None, _ptr(phi_corr), _ptr(b_phi_corr), _ptr(psi_inout)))

    def close(self):
        if self.h:
            lib().mi_mules_destroy(self.h)
            self.h = C.c_void_p()


class Interface:
    """The curvature's row pass on one mesh (mi_interface_create): boundary a GradBoundary or None (no boundary faces); it must stay open as
    long as the handle is used."""

    def __init__(self, addr: Addressing, boundary=None):
        self.addr, self.boundary = addr, boundary
        self.h = C.c_void_p()
        _chk(lib().mi_interface_create(addr.h, boundary.h if boundary is not None else None, C.byref(self.h)))

    def curvature(self, nhatf, vol, K_out, b_nhatf=None):
        """K = -fvc::div(nHatf) in one launch (mi_interface_curvature): b_nhatf the patch-ordered boundary faces"""
        _chk(lib().mi_interface_curvature(self.h, _ptr(nhatf), _ptr(b_nhatf), _ptr(vol), _ptr(K_out)))

    def close(self):
        if self.h:
            lib().mi_interface_destroy(self.h)
            self.h = C.c_void_p()


class KeCoeffs(C.Structure):
    """mi_ke_coeffs (include/mi_ldu.h)"""
    _fields_ = [(name, C.c_double) for name in ("Cmu", "C1", "C2", "sigmaEps", "kappa", "E", "Cmu25", "Cmu75", "yPlusLam")]


def ke_coeffs(Cmu=0.09, C1=1.44, C2=1.92, sigmaEps=1.3, kappa=0.41, E=9.8) -> KeCoeffs:
    """mi_ke_coeffs_init: kEpsilon's coefficients with Cmu25, Cmu75 and yPlusLam derived (host only, no GPU)"""
    out = KeCoeffs()
    _chk(lib().mi_ke_coeffs_init(C.c_double(Cmu), C.c_double(C1), C.c_double(C2), C.c_double(sigmaEps), C.c_double(kappa), C.c_double(E), C.byref(out)))
    return out


class LesCoeffs(C.Structure):
    """mi_les_coeffs (include/mi_ldu.h)"""
    _fields_ = [("ck", C.c_double), ("ce", C.c_double)]


def les_coeffs(ck=0.094, ce=1.048) -> LesCoeffs:
    """mi_les_coeffs_init: ck and ce of Smagorinsky / oneEqEddy (host only, no GPU)"""
    out = LesCoeffs()
    _chk(lib().mi_les_coeffs_init(C.c_double(ck), C.c_double(ce), C.byref(out)))
    return out


class KeWall(C.Structure):
    """mi_ke_wall (include/mi_ldu.h)"""
    _fields_ = [("k_dev", C.c_void_p), ("u_dev", C.c_void_p * 3), ("b_uw_dev", C.c_void_p * 3), ("b_delta_coeffs_dev", C.c_void_p),
                ("b_y_dev", C.c_void_p), ("b_nuw_dev", C.c_void_p), ("b_nutw_dev", C.c_void_p), ("g_inout_dev", C.c_void_p),
                ("eps_inout_dev", C.c_void_p), ("b_eps_out_dev", C.c_void_p), ("b_pow_out_dev", C.c_void_p)]


class Average:
    """fvc::average on one mesh (mi_average_create): keeps surfaceSum(magSf) per cell.  boundary a GradBoundary or None (no boundary faces); it
    must stay open as long as the handle is used.  mag_sf internal faces, b_mag_sf the patch-ordered boundary faces."""

    def __init__(self, addr: Addressing, boundary, mag_sf, b_mag_sf=None):
        self.addr, self.boundary = addr, boundary
        self.h = C.c_void_p()
        _chk(lib().mi_average_create(addr.h, boundary.h if boundary is not None else None, _ptr(mag_sf), _ptr(b_mag_sf), C.byref(self.h)))

    def fvc_average(self, mag_sf, ssf, out, b_mag_sf=None, b_ssf=None):
        """out = surfaceSum(magSf*ssf)/surfaceSum(magSf) in one row pass (mi_fvc_average)"""
        _chk(lib().mi_fvc_average(self.h, _ptr(mag_sf), _ptr(b_mag_sf), _ptr(ssf), _ptr(b_ssf), _ptr(out)))

    def bound(self, lower_bound, lam, mag_sf, vsf_inout, b_mag_sf=None, b_face=None):
        """bound.C:45-54 on the internal field in one row pass (mi_bound): b_face the boundary values of linearInterpolate(max(vsf, lb))"""
        _chk(lib().mi_bound(self.h, C.c_double(lower_bound), _ptr(lam), _ptr(mag_sf), _ptr(b_mag_sf), _ptr(b_face), _ptr(vsf_inout)))

    def les_simple_filter(self, lam, mag_sf, vf, out, b_mag_sf=None, b_face=None, n_cmpt=None):
        """out[k] = surfaceSum(magSf*interpolate(vf[k]))/surfaceSum(magSf) for up to nine components in one row pass (mi_les_simple_filter):
        vf, out and b_face lists of arrays (b_face the boundary face values of the unfiltered components); n_cmpt defaults to len(vf)"""
        nc = next((len(x) for x in (vf, out, b_face) if x is not None), 0) if n_cmpt is None else n_cmpt
        _chk(lib().mi_les_simple_filter(self.h, C.c_int(nc), _ptr(lam), _ptr(mag_sf), _ptr(b_mag_sf), _ptrs(vf, 9), _ptrs(b_face, 9), _ptrs(out, 9)))

    def close(self):
        if self.h:
            lib().mi_average_destroy(self.h)
            self.h = C.c_void_p()


class DeviceLabels:
    """int32 labels on the device that a handle owns, in the shape Assembly.set_values takes its cell_labels"""

    def __init__(self, n, address, owner):
        self.n, self.address, self.owner = int(n), int(address or 0), owner

    def numel(self):
        return self.n

    def data_ptr(self):
        return self.address

    def is_contiguous(self):
        return True

    def element_size(self):
        return 4


class KEpsilon:
    """The wall cells of one mesh (mi_ke_create): boundary a GradBoundary, patch_is_wall one flag per patch (a coupled patch is refused).
    The boundary must stay open as long as the handle is used."""

    def __init__(self, addr: Addressing, boundary, patch_is_wall: Sequence):
        self.addr, self.boundary = addr, boundary
        flags = (C.c_int32 * max(len(patch_is_wall), 1))(*[int(bool(x)) for x in patch_is_wall])
        self.h = C.c_void_p()
        _chk(lib().mi_ke_create(addr.h, boundary.h if boundary is not None else None, flags, C.byref(self.h)))

    def wall_cell_labels(self):
        """-> the labels of the unique wall cells, ascending, on the device and owned by the handle (mi_ke_wall_cell_labels): what
        Assembly.set_values takes for boundaryManipulate"""
        n, p = C.c_int32(0), C.c_void_p()
        _chk(lib().mi_ke_wall_cell_labels(self.h, C.byref(n), C.byref(p)))
        return DeviceLabels(n.value, p.value, self)

    def wall_cells(self, coeffs: KeCoeffs, k, u, b_uw, b_delta_coeffs, b_y, b_nuw, b_nutw, g_inout, eps_inout, b_eps_out, b_pow_out=None):
        """epsilon.boundaryField().updateCoeffs() for every wall patch in one launch (mi_ke_wall_cells): u / b_uw [x, y, z], every b_* array
        patch-ordered over the boundary"""
        x = KeWall()
        x.k_dev = _ptr(k).value
        for d in range(3):
            x.u_dev[d] = _ptr(None if u is None else u[d]).value
            x.b_uw_dev[d] = _ptr(None if b_uw is None else b_uw[d]).value
        x.b_delta_coeffs_dev, x.b_y_dev, x.b_nuw_dev, x.b_nutw_dev = (_ptr(t).value for t in (b_delta_coeffs, b_y, b_nuw, b_nutw))
        x.g_inout_dev, x.eps_inout_dev, x.b_eps_out_dev, x.b_pow_out_dev = (_ptr(t).value for t in (g_inout, eps_inout, b_eps_out, b_pow_out))
        _chk(lib().mi_ke_wall_cells(self.h, C.byref(coeffs) if coeffs is not None else None, C.byref(x)))

    def wall_values(self, eps, values_out):
        """values_out[i] = eps[label[i]] (mi_ke_wall_values): the values of boundaryManipulate's setValues"""
        _chk(lib().mi_ke_wall_values(self.h, _ptr(eps), _ptr(values_out)))

    def nut_wall(self, coeffs: KeCoeffs, k, b_y, b_nuw, b_nutw_out, b_log_out=None):
        """nutkWallFunction::calcNut on every wall face in one launch (mi_ke_nut_wall)"""
        _chk(lib().mi_ke_nut_wall(self.h, C.byref(coeffs) if coeffs is not None else None, _ptr(k), _ptr(b_y), _ptr(b_nuw), _ptr(b_nutw_out), _ptr(b_log_out)))

    def sst_wall_cells(self, coeffs: "SstCoeffs", k, u, b_uw, b_delta_coeffs, b_y, b_nuw, b_nutw, g_inout, omega_inout, b_omega_out):
        """omega.boundaryField().updateCoeffs() (omegaWallFunction) for every wall patch in one launch (mi_sst_wall_cells): the arrays of
        wall_cells"""
        x = SstWall()
        x.k_dev = _ptr(k).value
        for d in range(3):
            x.u_dev[d] = _ptr(None if u is None else u[d]).value
            x.b_uw_dev[d] = _ptr(None if b_uw is None else b_uw[d]).value
        x.b_delta_coeffs_dev, x.b_y_dev, x.b_nuw_dev, x.b_nutw_dev = (_ptr(t).value for t in (b_delta_coeffs, b_y, b_nuw, b_nutw))
        x.g_inout_dev, x.omega_inout_dev, x.b_omega_out_dev = (_ptr(t).value for t in (g_inout, omega_inout, b_omega_out))
        _chk(lib().mi_sst_wall_cells(self.h, C.byref(coeffs) if coeffs is not None else None, C.byref(x)))

    def sa_nut_spalding_wall(self, coeffs: "SaCoeffs", u, b_uw, b_delta_coeffs, b_y, b_nuw, b_nutw_inout, b_exp_out=None, b_iter_out=None):
        """nutUSpaldingWallFunction::calcNut with calcUTau's Newton loop on every wall face in one launch (mi_sa_nut_spalding_wall):
        b_nutw_inout the boundary values of nut (the wall faces are read and rewritten), b_exp_out 10 doubles per boundary face for the exp of
        every step taken, b_iter_out an int32 tensor per boundary face for the number of steps"""
        x = SaWall()
        for d in range(3):
            x.u_dev[d] = _ptr(None if u is None else u[d]).value
            x.b_uw_dev[d] = _ptr(None if b_uw is None else b_uw[d]).value
        x.b_delta_coeffs_dev, x.b_y_dev, x.b_nuw_dev, x.b_nutw_inout_dev, x.b_exp_out_dev_or_null = \
            (_ptr(t).value for t in (b_delta_coeffs, b_y, b_nuw, b_nutw_inout, b_exp_out))
        if b_iter_out is not None:
            assert b_iter_out.is_contiguous() and b_iter_out.element_size() == 4
            x.b_iter_out_dev_or_null = b_iter_out.data_ptr()
        _chk(lib().mi_sa_nut_spalding_wall(self.h, C.byref(coeffs) if coeffs is not None else None, C.byref(x)))

    def close(self):
        if self.h:
            lib().mi_ke_destroy(self.h)
            self.h = C.c_void_p()


SST_MODEL = ("alphaK1", "alphaK2", "alphaOmega1", "alphaOmega2", "gamma1", "gamma2", "beta1", "beta2", "betaStar", "a1", "b1", "c1")
SST_WALL = ("Cmu", "kappa", "E", "wallBeta1")


class SstCoeffs(C.Structure):
    """mi_sst_coeffs (include/mi_ldu.h)"""
    _fields_ = [(name, C.c_double) for name in SST_MODEL + SST_WALL + ("twoAlphaOmega2", "fourAlphaOmega2", "invBetaStar", "twoInvBetaStar",
                                                                       "c1a1BetaStar", "c1BetaStar", "dAlphaK", "dAlphaOmega", "dBeta", "dGamma",
                                                                       "Cmu25", "yPlusLam")]


def sst_coeffs(**given) -> SstCoeffs:
    """mi_sst_coeffs_init: kOmegaSST's coefficients (SST_MODEL) and its wall function's (SST_WALL) by name, the reference's defaults for the
    rest, with the host-formed products derived (host only, no GPU)"""
    unknown = set(given) - set(SST_MODEL) - set(SST_WALL)
    if unknown:
        raise TypeError("sst_coeffs: unknown coefficient " + ", ".join(sorted(unknown)))
    base = SstCoeffs()
    _chk(lib().mi_sst_coeffs_init(None, None, C.byref(base)))
    model = (C.c_double * 12)(*[float(given.get(name, getattr(base, name))) for name in SST_MODEL])
    wall = (C.c_double * 4)(*[float(given.get(name, getattr(base, name))) for name in SST_WALL])
    out = SstCoeffs()
    _chk(lib().mi_sst_coeffs_init(model, wall, C.byref(out)))
    return out


class ThermoModel(C.Structure):
    """mi_thermo_model (include/mi_ldu.h)"""
    _fields_ = [(name, C.c_int32) for name in ("energy", "thermo", "transport", "reserved")] + \
               [(name, C.c_double) for name in ("W", "Cp", "Cv", "Hf", "Tlow", "Thigh", "Tcommon")] + \
               [("highCpCoeffs", C.c_double * 7), ("lowCpCoeffs", C.c_double * 7)] + \
               [(name, C.c_double) for name in ("mu", "Pr", "As", "Ts", "R", "cpMcv", "CpW", "CvW", "HfW", "cpE", "rPr")] + \
               [("highH", C.c_double * 4), ("lowH", C.c_double * 4), ("hc", C.c_double)]


THERMO_ENERGY = {"sensibleEnthalpy": 0, "h": 0, "sensibleInternalEnergy": 1, "e": 1}
THERMO_THERMO = {"hConst": 0, "eConst": 1, "janaf": 2}
THERMO_TRANSPORT = {"const": 0, "sutherland": 1}
THERMO_PROPERTIES = {"Cp": 0, "Cv": 1, "gamma": 2, "Cpv": 3, "CpByCpv": 4, "kappa": 5}
# air: the defaults of thermo_model (the janaf set is the two-range fit of the thermophysicalProperties of the combustion tutorials)
THERMO_DEFAULTS = dict(
    energy="sensibleEnthalpy", thermo="hConst", transport="const", W=28.9, Cp=1007.0, Cv=719.3, Hf=0.0, mu=1.84e-05, Pr=0.7, As=1.4792e-06, Ts=116.0,
    Tlow=200.0, Thigh=6000.0, Tcommon=1000.0,
    highCpCoeffs=(3.08792717, 0.00124597184, -4.23718945e-07, 6.74774789e-11, -3.97076972e-15, -995.262755, 5.9596093),
    lowCpCoeffs=(3.5683962, -0.000678729429, 1.55371476e-06, -3.2993706e-12, -4.66395387e-13, -1062.34659, 3.71582965))


def thermo_model(**given) -> ThermoModel:
    """mi_thermo_model_init: one pure-mixture thermoType by name -- energy ("sensibleEnthalpy" / "h", "sensibleInternalEnergy" / "e"), thermo
    ("hConst", "eConst", "janaf"), transport ("const", "sutherland"), W and the dictionary's per-mass numbers of the chosen parts, air's
    (THERMO_DEFAULTS) for the rest -- with the host-formed members derived (host only, no GPU)"""
    unknown = set(given) - set(THERMO_DEFAULTS)
    if unknown:
        raise TypeError("thermo_model: unknown name " + ", ".join(sorted(unknown)))
    g = dict(THERMO_DEFAULTS, **given)
    for name, table in (("energy", THERMO_ENERGY), ("thermo", THERMO_THERMO), ("transport", THERMO_TRANSPORT)):
        if not isinstance(g[name], int) and g[name] not in table:
            raise MiError(f"thermo_model: unknown {name} {g[name]!r}")
    e, th, tr = [g[name] if isinstance(g[name], int) else table[g[name]]
                 for name, table in (("energy", THERMO_ENERGY), ("thermo", THERMO_THERMO), ("transport", THERMO_TRANSPORT))]
    if th == 2:
        if len(g["highCpCoeffs"]) != 7 or len(g["lowCpCoeffs"]) != 7:
            raise MiError("thermo_model: janaf takes seven high and seven low coefficients")
        tv = [g["Tlow"], g["Thigh"], g["Tcommon"], *g["highCpCoeffs"], *g["lowCpCoeffs"]]
    else:
        tv = [g["Cv"] if th == 1 else g["Cp"], g["Hf"]]
    xv = [g["As"], g["Ts"]] if tr == 1 else [g["mu"], g["Pr"]]
    out = ThermoModel()
    _chk(lib().mi_thermo_model_init(C.c_int(e), C.c_int(th), C.c_int(tr), C.c_double(g["W"]), (C.c_double * len(tv))(*[float(v) for v in tv]),
                                    (C.c_double * 2)(*[float(v) for v in xv]), C.byref(out)))
    return out


class SstWall(C.Structure):
    """mi_sst_wall (include/mi_ldu.h)"""
    _fields_ = [("k_dev", C.c_void_p), ("u_dev", C.c_void_p * 3), ("b_uw_dev", C.c_void_p * 3), ("b_delta_coeffs_dev", C.c_void_p),
                ("b_y_dev", C.c_void_p), ("b_nuw_dev", C.c_void_p), ("b_nutw_dev", C.c_void_p), ("g_inout_dev", C.c_void_p),
                ("omega_inout_dev", C.c_void_p), ("b_omega_out_dev", C.c_void_p)]


class SstBlendArrays(C.Structure):
    """mi_sst_blend_arrays (include/mi_ldu.h)"""
    _fields_ = [("grad_k_dev", C.c_void_p * 3), ("grad_omega_dev", C.c_void_p * 3)] + \
               [(name, C.c_void_p) for name in ("k_dev", "omega_dev", "y_dev", "nut_dev", "s2_dev", "nu_dev_or_null")] + [("nu_value", C.c_double)] + \
               [(name, C.c_void_p) for name in ("f1_out_dev", "su_out_dev", "sp_out_dev", "susp_out_dev", "domega_out_dev", "dk_out_dev",
                                                "cdkomega_out_dev_or_null", "arg1_out_dev_or_null", "f23_out_dev_or_null", "tanh3_out_dev_or_null")]


SA_MODEL = ("sigmaNut", "kappa", "Cb1", "Cb2", "Cw2", "Cw3", "Cv1", "Cv2", "CDES", "ck", "fwStar", "cl", "ct")
SA_WALL = ("wallKappa", "E")
SA_DERIVED = ("Cw1", "Cb2BySigmaNut", "Cv1_3", "Cw3_6", "onePlusCw3_6", "invCv2", "ct2", "cl2", "psiDen", "psiCoeff", "invE", "sqrt2")
SA_KINDS = {"RAS": 0, "DES": 1, "DDES": 2, "IDDES": 3}
SA_OPTIONAL = ("s", "dtilda", "stilda", "pow_fw", "tanh_fd", "exp", "pow_hill_pos", "pow_hill_neg", "tanh_ft", "pow_fl", "tanh_fl")


class SaCoeffs(C.Structure):
    """mi_sa_coeffs (include/mi_ldu.h)"""
    _fields_ = [(name, C.c_double) for name in SA_MODEL + SA_WALL + SA_DERIVED]


def sa_coeffs(**given) -> SaCoeffs:
    """mi_sa_coeffs_init: the Spalart-Allmaras coefficients (SA_MODEL) and the wall function's (SA_WALL) by name, the reference's defaults for
    the rest, with the host-formed products derived (host only, no GPU)"""
    unknown = set(given) - set(SA_MODEL) - set(SA_WALL)
    if unknown:
        raise TypeError("sa_coeffs: unknown coefficient " + ", ".join(sorted(unknown)))
    base = SaCoeffs()
    _chk(lib().mi_sa_coeffs_init(None, None, C.byref(base)))
    model = (C.c_double * 13)(*[float(given.get(name, getattr(base, name))) for name in SA_MODEL])
    wall = (C.c_double * 2)(*[float(given.get(name, getattr(base, name))) for name in SA_WALL])
    out = SaCoeffs()
    _chk(lib().mi_sa_coeffs_init(model, wall, C.byref(out)))
    return out


class SaCells(C.Structure):
    """mi_sa_cells (include/mi_ldu.h)"""
    _fields_ = [("nutilda_dev", C.c_void_p), ("grad_dev", C.c_void_p * 9), ("grad_nutilda_dev", C.c_void_p * 3), ("y_dev", C.c_void_p),
                ("nu_dev_or_null", C.c_void_p), ("nu_value", C.c_double), ("delta_dev", C.c_void_p), ("nusgs_dev", C.c_void_p), ("hmax_dev", C.c_void_p)] + \
               [(name, C.c_void_p) for name in ("su_grad_out_dev", "su_prod_out_dev", "sp_out_dev", "dnu_out_dev", "fv1_out_dev")] + \
               [(name + "_out_dev_or_null", C.c_void_p) for name in SA_OPTIONAL]


class SaWall(C.Structure):
    """mi_sa_wall (include/mi_ldu.h)"""
    _fields_ = [("u_dev", C.c_void_p * 3), ("b_uw_dev", C.c_void_p * 3), ("b_delta_coeffs_dev", C.c_void_p), ("b_y_dev", C.c_void_p),
                ("b_nuw_dev", C.c_void_p), ("b_nutw_inout_dev", C.c_void_p), ("b_exp_out_dev_or_null", C.c_void_p), ("b_iter_out_dev_or_null", C.c_void_p)]


class Assembly:
    """fvm::div / fvm::laplacian / negSumDiag / relax ... on caller-order arrays of an Addressing."""

    def __init__(self, addr: Addressing):
        self.addr = addr

    def row_face_op(self, kind: int, lower, upper, inout):
        _chk(lib().mi_row_face_op(self.addr.h, int(kind), _ptr(lower), _ptr(upper), _ptr(inout)))

    def fvm_laplacian(self, delta_coeffs, gamma_magsf, upper_out, diag_out):
        _chk(lib().mi_fvm_laplacian(self.addr.h, _ptr(delta_coeffs), _ptr(gamma_magsf), _ptr(upper_out), _ptr(diag_out)))

    def fvm_div(self, weights, face_flux, lower_out, upper_out, diag_out):
        _chk(lib().mi_fvm_div(self.addr.h, _ptr(weights), _ptr(face_flux), _ptr(lower_out), _ptr(upper_out), _ptr(diag_out)))

    def surface_integrate(self, ssf, vol, ivf):
        _chk(lib().mi_surface_integrate(self.addr.h, _ptr(ssf), _ptr(vol), _ptr(ivf)))

    def face_interpolate(self, lam, phi, sf):
        _chk(lib().mi_face_interpolate(self.addr.h, _ptr(lam), _ptr(phi), _ptr(sf)))

    def fvm_ddt_euler(self, r_delta_t, rho, vol, psi_old, diag_out, source_out):
        _chk(lib().mi_fvm_ddt_euler(self.addr.ctx.h, C.c_int64(vol.numel()), C.c_double(r_delta_t), C.c_double(rho), _ptr(vol), _ptr(psi_old),
                                    _ptr(diag_out), _ptr(source_out)))

    def fvm_ddt_euler_rho(self, r_delta_t, rho, rho_old, vol, psi_old, diag_out, source_out):
        """fvm::ddt(rho, vf) with a density field (EulerDdtScheme.C:403-440)"""
        _chk(lib().mi_fvm_ddt_euler_rho(self.addr.ctx.h, C.c_int64(vol.numel()), C.c_double(r_delta_t), _ptr(rho), _ptr(rho_old), _ptr(vol),
                                        _ptr(psi_old), _ptr(diag_out), _ptr(source_out)))

    def fvm_su(self, vol, su, source_inout):
        _chk(lib().mi_fvm_su(self.addr.ctx.h, C.c_int64(vol.numel()), _ptr(vol), _ptr(su), _ptr(source_inout)))

    def fvm_sp(self, vol, sp, diag_inout):
        """sp: a cell field or a number (fvmSup.C:100-170)"""
        if isinstance(sp, (int, float)):
            _chk(lib().mi_fvm_sp(self.addr.ctx.h, C.c_int64(vol.numel()), _ptr(vol), None, C.c_double(sp), _ptr(diag_inout)))
        else:
            _chk(lib().mi_fvm_sp(self.addr.ctx.h, C.c_int64(vol.numel()), _ptr(vol), _ptr(sp), C.c_double(0.0), _ptr(diag_inout)))

    def fvm_susp(self, vol, susp, vf, diag_inout, source_inout):
        _chk(lib().mi_fvm_susp(self.addr.ctx.h, C.c_int64(vol.numel()), _ptr(vol), _ptr(susp), _ptr(vf), _ptr(diag_inout), _ptr(source_inout)))

    def flux_div(self, lam, sf, v, phi_out, div_out, cell_scale=None, add_a=None, add_b=None, vol=None):
        """phi = Sf & interpolate([cell_scale *] v) [+ add_a [* add_b]] and div = surfaceIntegrate(phi) [/ vol] in one row pass"""
        _chk(lib().mi_flux_div(self.addr.h, _ptr(lam), _ptr(sf[0]), _ptr(sf[1]), _ptr(sf[2]), _ptr(v[0]), _ptr(v[1]), _ptr(v[2]), _ptr(cell_scale),
                               _ptr(add_a), _ptr(add_b), _ptr(phi_out), _ptr(vol), _ptr(div_out)))

    def ddt_phi_corr(self, r_delta_t, lam, sf, u_old, rho_old, phi_old, out):
        """fvc::ddtCorr(rho, U, phi) on the internal faces (EulerDdtScheme.C:663-720; rho_old None: :523-551)"""
        _chk(lib().mi_ddt_phi_corr(self.addr.h, C.c_double(r_delta_t), _ptr(lam), _ptr(sf[0]), _ptr(sf[1]), _ptr(sf[2]), _ptr(u_old[0]), _ptr(u_old[1]),
                                   _ptr(u_old[2]), _ptr(rho_old), _ptr(phi_old), _ptr(out)))

    def fvm_ddt_backward(self, r_delta_t, coeffs, vol, psi_old, psi_old_old, diag_out, source_out, rho_value=1.0, rho=None, rho_old=None, rho_old_old=None):
        """fvm::ddt([rho,] vf), backward (backwardDdtScheme.C:456-607): coeffs from ddt_backward_coeffs; rho / rho_old / rho_old_old: a density
        field (all three) or none (the constant rho_value)"""
        _chk(lib().mi_fvm_ddt_backward(self.addr.ctx.h, C.c_int64(vol.numel()), C.c_double(r_delta_t), (C.c_double * 3)(*coeffs), C.c_double(rho_value),
                                       _ptr(rho), _ptr(rho_old), _ptr(rho_old_old), _ptr(vol), _ptr(psi_old), _ptr(psi_old_old), _ptr(diag_out), _ptr(source_out)))

    def fvc_ddt_backward(self, r_delta_t, coeffs, vf, vf_old, vf_old_old, out, rho_value=1.0, rho=None, rho_old=None, rho_old_old=None):
        """fvc::ddt([rho,] vf), backward (backwardDdtScheme.C:196-207, 268-280, 343-355)"""
        _chk(lib().mi_fvc_ddt_backward(self.addr.ctx.h, C.c_int64(vf.numel()), C.c_double(r_delta_t), (C.c_double * 3)(*coeffs), C.c_double(rho_value),
                                       _ptr(rho), _ptr(rho_old), _ptr(rho_old_old), _ptr(vf), _ptr(vf_old), _ptr(vf_old_old), _ptr(out)))

    def ddt_phi_corr_backward(self, r_delta_t, coeffs, lam, sf, u_old, u_old_old, rho_old, rho_old_old, phi_old, phi_old_old, out):
        """fvc::ddtCorr([rho,] U, phi), backward, on the internal faces (backwardDdtScheme.C:724-765, 868-950; rho_old / rho_old_old both None or both given)"""
        _chk(lib().mi_ddt_phi_corr_backward(self.addr.h, C.c_double(r_delta_t), (C.c_double * 3)(*coeffs), _ptr(lam), _ptr(sf[0]), _ptr(sf[1]), _ptr(sf[2]),
                                            _ptr(u_old[0]), _ptr(u_old[1]), _ptr(u_old[2]), _ptr(u_old_old[0]), _ptr(u_old_old[1]), _ptr(u_old_old[2]),
                                            _ptr(rho_old), _ptr(rho_old_old), _ptr(phi_old), _ptr(phi_old_old), _ptr(out)))

    def ddt_cn_update(self, r_dt_coef0, oc, psi_old, psi_old_old, ddt0_inout, rho_value=1.0, rho_old=None, rho_old_old=None):
        """the ddt0 update of CrankNicolson (CrankNicolsonDdtScheme.C:417-418, 507-508, 603-607), IN PLACE, of 1..4 fields (lists of tensors) in one
        launch; rho_old / rho_old_old: a density field (both) or none (the constant rho_value)"""
        k = len(ddt0_inout)
        assert len(psi_old) == k and len(psi_old_old) == k, "one old and one old-old field per ddt0 field"
        arr = lambda xs: (C.c_void_p * max(k, 1))(*[_ptr(x) for x in xs])
        n = next((x.numel() for x in (*ddt0_inout, *psi_old, *psi_old_old) if x is not None), 0)
        _chk(lib().mi_ddt_cn_update(self.addr.ctx.h, C.c_int64(n), C.c_int32(k), C.c_double(r_dt_coef0), C.c_double(oc),
                                    C.c_double(rho_value), _ptr(rho_old), _ptr(rho_old_old), arr(psi_old), arr(psi_old_old), arr(ddt0_inout)))

    def fvm_ddt_cn(self, r_dt_coef, oc, vol, psi_old, ddt0, diag_out, source_out, rho_value=1.0, rho=None, rho_old=None):
        """fvm::ddt([rho,] vf), CrankNicolson (CrankNicolsonDdtScheme.C:755-1003): ddt0 already updated for this time step"""
        _chk(lib().mi_fvm_ddt_cn(self.addr.ctx.h, C.c_int64(vol.numel()), C.c_double(r_dt_coef), C.c_double(oc), C.c_double(rho_value), _ptr(rho), _ptr(rho_old),
                                 _ptr(vol), _ptr(psi_old), _ptr(ddt0), _ptr(diag_out), _ptr(source_out)))

    def fvc_ddt_cn(self, r_dt_coef, oc, vf, vf_old, ddt0, out, rho_value=1.0, rho=None, rho_old=None):
        """fvc::ddt([rho,] vf), CrankNicolson (CrankNicolsonDdtScheme.C:426, 516, 615-616)"""
        _chk(lib().mi_fvc_ddt_cn(self.addr.ctx.h, C.c_int64(vf.numel()), C.c_double(r_dt_coef), C.c_double(oc), C.c_double(rho_value), _ptr(rho), _ptr(rho_old),
                                 _ptr(vf), _ptr(vf_old), _ptr(ddt0), _ptr(out)))

    def fvm_ddt_local(self, r_delta_t, vol, psi_old, diag_out, source_out, rho_value=1.0, rho=None, rho_old=None):
        """fvm::ddt([rho,] vf), localEuler / CoEuler (localEulerDdtScheme.C:339-445): r_delta_t the rDeltaT CELL field"""
        _chk(lib().mi_fvm_ddt_local(self.addr.ctx.h, C.c_int64(vol.numel()), _ptr(r_delta_t), C.c_double(rho_value), _ptr(rho), _ptr(rho_old), _ptr(vol),
                                    _ptr(psi_old), _ptr(diag_out), _ptr(source_out)))

    def fvc_ddt_local(self, r_delta_t, vf, vf_old, out, rho_value=1.0, rho=None, rho_old=None):
        """fvc::ddt([rho,] vf), localEuler / CoEuler (localEulerDdtScheme.C:149-157, 200-209, 255-264)"""
        _chk(lib().mi_fvc_ddt_local(self.addr.ctx.h, C.c_int64(vf.numel()), _ptr(r_delta_t), C.c_double(rho_value), _ptr(rho), _ptr(rho_old), _ptr(vf),
                                    _ptr(vf_old), _ptr(out)))

    def ddt_phi_corr_local(self, r_delta_t, lam, sf, u_old, phi_old, out):
        """fvc::ddtCorr(U, phi), localEuler / CoEuler, on the internal faces (localEulerDdtScheme.C:531-560): rDeltaT interpolated per face"""
        _chk(lib().mi_ddt_phi_corr_local(self.addr.h, _ptr(r_delta_t), _ptr(lam), _ptr(sf[0]), _ptr(sf[1]), _ptr(sf[2]), _ptr(u_old[0]), _ptr(u_old[1]),
                                         _ptr(u_old[2]), _ptr(phi_old), _ptr(out)))

    def co_face_r_delta_t(self, delta_coeffs, mag_sf, phi, delta_t, max_co, out, rho_face=None):
        """CoEuler's face rDeltaT max(Co/maxCo, 1)/deltaT as a streaming pass (a patch's faces; CoEulerDdtScheme.C:125-167); rho_face: mass flux"""
        _chk(lib().mi_co_face_r_delta_t(self.addr.ctx.h, C.c_int64(out.numel()), _ptr(delta_coeffs), _ptr(mag_sf), _ptr(phi), _ptr(rho_face),
                                        C.c_double(delta_t), C.c_double(max_co), _ptr(out)))

    def co_r_delta_t(self, delta_coeffs, mag_sf, phi, delta_t, max_co, out, lam=None, rho_old=None):
        """CoEuler's cell rDeltaT over the internal faces in one row pass (CoEulerDdtScheme.C:61-94); lam and rho_old together: mass flux.  The
        patches follow with Patch.max"""
        _chk(lib().mi_co_r_delta_t(self.addr.h, _ptr(delta_coeffs), _ptr(mag_sf), _ptr(phi), _ptr(lam), _ptr(rho_old), C.c_double(delta_t),
                                   C.c_double(max_co), _ptr(out)))

    def upwind_weights(self, face_flux, w_out):
        _chk(lib().mi_upwind_weights(self.addr.ctx.h, C.c_int64(face_flux.numel()), _ptr(face_flux), _ptr(w_out)))

    def limited_linear_weights(self, k, cd_weights, face_flux, phi, grad, centres, w_out, limiter_out=None):
        _chk(lib().mi_limited_linear_weights(self.addr.h, C.c_double(k), _ptr(cd_weights), _ptr(face_flux), _ptr(phi), _ptr(grad[0]), _ptr(grad[1]),
                                             _ptr(grad[2]), _ptr(centres[0]), _ptr(centres[1]), _ptr(centres[2]), _ptr(w_out), _ptr(limiter_out)))

    def gauss_grad(self, sf, ssf, vol, grad_out):
        _chk(lib().mi_gauss_grad(self.addr.h, _ptr(sf[0]), _ptr(sf[1]), _ptr(sf[2]), _ptr(ssf), _ptr(vol), _ptr(grad_out[0]), _ptr(grad_out[1]),
                                 _ptr(grad_out[2])))

    def sngrad_correction_flux(self, corr_vecs, weights, grad, gamma_magsf, out):
        """gammaMagSf * (nonOrthCorrectionVectors & interpolate(grad)) on the internal faces (gaussLaplacianSchemes.C:64-90)"""
        _chk(lib().mi_sngrad_correction_flux(self.addr.h, _ptr(corr_vecs[0]), _ptr(corr_vecs[1]), _ptr(corr_vecs[2]), _ptr(weights), _ptr(grad[0]),
                                             _ptr(grad[1]), _ptr(grad[2]), _ptr(gamma_magsf), _ptr(out)))

    def sngrad_limited_correction_flux(self, limit_coeff, corr_vecs, weights, delta_coeffs, vf, grad, gamma_magsf, out, limiter_out=None):
        """[gammaMagSf *] limiter*correction of the `limited` snGrad scheme on the internal faces in one face pass (limitedSnGrad.C:58-84): vf 1 or
        3 cell arrays, grad 3 or 9 (grad[3*j + d] = d(vf_j)/dx_d), out one face array per component, limiter_out one face array or None"""
        _chk(lib().mi_sngrad_limited_correction_flux(self.addr.h, C.c_int32(len(vf)), C.c_double(limit_coeff), _ptr(corr_vecs[0]), _ptr(corr_vecs[1]),
                                                     _ptr(corr_vecs[2]), _ptr(weights), _ptr(delta_coeffs), _ptrs(vf), _ptrs(grad), _ptr(gamma_magsf), _ptrs(out),
                                                     _ptr(limiter_out)))

    def div_dev_tgrad(self, kind, lam, sf, visc, grad, face_out, div_out, vol=None):
        """fvc::div(visc*dev(T(grad))) ("dev": divDevReff) | fvc::div(visc*dev2(T(grad))) ("dev2": divDevRhoReff) on the internal faces in one face
        pass and one row pass (mi_fvc_div_dev_tgrad): grad 9 cell arrays (grad[3*j + k] = d(U_j)/dx_k), face_out 3 face arrays (kept for the
        patch sums and flux()), div_out 3 cell arrays [/ vol]"""
        _chk(lib().mi_fvc_div_dev_tgrad(self.addr.h, C.c_int32(_dev_kind(kind)), _ptr(lam), _ptr(sf[0]), _ptr(sf[1]), _ptr(sf[2]), _ptr(visc), _ptrs(grad),
                                        _ptr(vol), _ptrs(face_out), _ptrs(div_out)))

    def linear_upwind_correction(self, face_flux, cf, c, grad, out, scale=1.0):
        """faceFlux*correction(vf) of linearUpwind (scale 1) / LUST (scale 0.25) on the internal faces, one face pass for len(out) <= 4 components
        (linearUpwind.C:33-47); grad one [gx, gy, gz] per component"""
        k = div_correction(cf, c, grad, scale)
        o = (C.c_void_p * max(len(out), 1))(*[_ptr(x) for x in out])
        _chk(lib().mi_linear_upwind_correction(self.addr.h, C.byref(k), C.c_int32(len(out)), _ptr(face_flux), o))

    def limited_weights(self, lim, cd_weights, face_flux, phi, grad, centres, w_out, limiter_out=None):
        """a limited scheme's weights on the internal faces in one face pass (mi_limited_weights): lim a Limiter or a scheme name, phi 1 or 3
        cell arrays, grad 3 or 9 (grad[3*j + k] = d(phi_j)/dx_k), centres [x, y, z]"""
        lim = limiter(lim) if isinstance(lim, str) else lim
        _chk(lib().mi_limited_weights(self.addr.h, C.byref(lim), _ptr(cd_weights), _ptr(face_flux), _ptrs(phi), _ptrs(grad), _ptrs(centres), _ptr(w_out),
                                      _ptr(limiter_out)))

    def filtered_weights(self, lim, cd_weights, face_flux, phi, grad, centres, w_out, limiter_out=None):
        """a filtered scheme's weights on the internal faces in one face pass (mi_filtered_weights): lim a FilteredLimiter or a scheme name
        ("filteredLinear2V 1 0"), the other arguments as limited_weights"""
        lim = filtered(lim) if isinstance(lim, str) else lim
        _chk(lib().mi_filtered_weights(self.addr.h, C.byref(lim), _ptr(cd_weights), _ptr(face_flux), _ptrs(phi), _ptrs(grad), _ptrs(centres), _ptr(w_out),
                                       _ptr(limiter_out)))

    def cubic_correction(self, geo, vf, grad, out, face_flux=None):
        """[faceFlux *] correction(vf) of cubic on the internal faces, one face pass for len(out) <= 4 components (mi_cubic_correction; cubic.H:111-184):
        geo a CubicGeometry, vf one cell array per component, grad one [gx, gy, gz] (Gauss linear) per component; face_flux None: the bare
        correction field of fvc::interpolate"""
        _chk(lib().mi_cubic_correction(self.addr.h, C.byref(geo), C.c_int32(len(out)), _ptrs(vf), _ptrs([g for gr in grad for g in gr]), _ptr(face_flux),
                                       _ptrs(out)))

    def limited_grad(self, lim, vf, centres, cf, grad, boundary=None, bvalue=None, bcf=None, limiter_out=None):
        """limits a Gauss linear gradient in place (mi_limited_grad): lim a GradLimiter or a scheme ("cellLimited Gauss linear 1"), vf 1 or 3
        cell arrays, centres / cf / bcf [x, y, z] (cells, internal faces, boundary faces), grad 3 or 9 (grad[3*j + k] = d(vf_j)/dx_k),
        boundary a GradBoundary (or None), bvalue one boundary-face array per component; limiter_out n_comp arrays (cellLimited), 1
        (faceLimited) or None"""
        lim = grad_limiter(lim) if isinstance(lim, str) else lim
        _chk(lib().mi_limited_grad(self.addr.h, C.byref(lim), boundary.h if boundary is not None else None, C.c_int32(len(vf)), _ptrs(vf),
                                   _ptrs(centres), _ptrs(cf), _ptrs(bvalue), _ptrs(bcf), _ptrs(grad), _ptrs(limiter_out)))

    def ls_grad(self, lsv, vf, grad_out, bvalue=None):
        """the leastSquares gradient's internal field in one row pass (mi_ls_grad): lsv an LsVectors of this addressing, vf 1 or 3 cell arrays,
        grad_out 3 or 9 (grad_out[3*j + k] = d(vf_j)/dx_k), bvalue one boundary-face array per component (patchNeighbourField on coupled
        patches, the boundary value elsewhere)"""
        if lsv.addr is not self.addr:
            raise MiError("ls_grad: the vectors were built for another addressing")
        _chk(lib().mi_ls_grad(lsv.h, C.c_int32(len(vf)), _ptrs(vf), _ptrs(bvalue), _ptrs(grad_out)))

    def surface_sum(self, ssf, out, mode="sum"):
        """fvc::surfaceSum over the internal faces, every term added on both sides (mi_surface_sum): mode "sum" | "mag" (the sum of |ssf|, as
        in CourantNo.H); the boundary faces follow per patch with Patch.add (fn 0 / fn 2)"""
        m = SURFACE_SUM_MODES.index(mode) if mode in SURFACE_SUM_MODES else int(mode)
        _chk(lib().mi_surface_sum(self.addr.h, C.c_int32(m), _ptr(ssf), _ptr(out)))

    def reconstruct(self, rc, ssf, out, b_ssf=None):
        """fvc::reconstruct of 1 to 4 face fluxes in one row pass (mi_fvc_reconstruct): rc a Reconstruct of this addressing, ssf one internal-
        face array per flux, b_ssf one boundary-face array per flux (None without boundary faces), out three cell arrays per flux
        (out[3*r + k] = component k of flux r's vector)"""
        if rc.addr is not self.addr:
            raise MiError("reconstruct: the handle was built for another addressing")
        _chk(lib().mi_fvc_reconstruct(rc.h, C.c_int32(len(ssf)), _ptrs(ssf), _ptrs(b_ssf), _ptrs(out)))

    def _mules(self, mu):
        if mu.addr is not self.addr:
            raise MiError("mules: the handle was built for another addressing")
        return mu

    def mules_begin(self, mu, form, fields, flux):
        """opens a MULES limiter on a Mules of this addressing (mi_mules_begin): form "limiter" (phi_bd, phi_corr and lambda as given) or
        "limit" (phi and phi_psi given; phi_bd, phi_corr and lambda = 1 written)"""
        self._mules(mu).begin(form, fields, flux)

    def mules_iterate(self, mu, n, fields, flux):
        """n limiter iterations, lambda in place (mi_mules_iterate); with coupled patches one at a time, vec_min on the two sides after each"""
        self._mules(mu).iterate(n, fields, flux)

    def mules_apply(self, mu, return_corr, fields, flux):
        """out = phi_bd + lambda*phi_corr, or lambda*phi_corr with return_corr (mi_mules_apply)"""
        self._mules(mu).apply(return_corr, fields, flux)

    def mules_limiter(self, mu, fields, flux, n_limiter_iter=3):
        self._mules(mu).limiter(fields, flux, n_limiter_iter)

    def mules_limit(self, mu, fields, flux, n_limiter_iter=3, return_corr=False):
        self._mules(mu).limit(fields, flux, n_limiter_iter, return_corr)

    def mules_explicit_solve(self, mu, fields, phi_psi, psi_out, b_phi_psi=None):
        self._mules(mu).explicit_solve(fields, phi_psi, psi_out, b_phi_psi)

    def mules_begin_corr(self, mu, form, fields, flux, extrema_coeff=0.0):
        """opens semi-implicit MULES' limiter (mi_mules_begin_corr): form "limiter" (lambda as given) or "limit" (lambda = 1); reads phi_corr,
        b_phi_corr and the current psi / rho; mules_iterate then takes the CMULES patch rule (it reads b_phi) and mules_apply(return_corr=True)
        may write phi_corr in place"""
        self._mules(mu).begin_corr(form, fields, flux, extrema_coeff)

    def mules_limiter_corr(self, mu, fields, flux, n_limiter_iter=3, extrema_coeff=0.0):
        self._mules(mu).limiter_corr(fields, flux, n_limiter_iter, extrema_coeff)

    def mules_limit_corr(self, mu, fields, flux, n_limiter_iter=3, extrema_coeff=0.0):
        self._mules(mu).limit_corr(fields, flux, n_limiter_iter, extrema_coeff)

    def mules_correct(self, mu, fields, phi_corr, psi_inout, b_phi_corr=None):
        self._mules(mu).correct(fields, phi_corr, psi_inout, b_phi_corr)

    def interface_compression_weights(self, cd_weights, face_flux, alpha, w_out, limiter_out=None):
        """the interfaceCompression scheme's weights on the internal faces in one face pass (mi_interface_compression_weights): the limiter
        from the two cell values of alpha, no gradient and no centres"""
        _chk(lib().mi_interface_compression_weights(self.addr.h, _ptr(cd_weights), _ptr(face_flux), _ptr(alpha), _ptr(w_out), _ptr(limiter_out)))

    def alpha_compression_flux(self, cd_weights, phir, alpha1, out):
        """fvc::flux(-fvc::flux(-phir, 1 - alpha1, interfaceCompression), alpha1, interfaceCompression) on the internal faces in one face pass
        (mi_alpha_compression_flux), the bits of the unfused sequence"""
        _chk(lib().mi_alpha_compression_flux(self.addr.h, _ptr(cd_weights), _ptr(phir), _ptr(alpha1), _ptr(out)))

    def interface_nhatf(self, delta_n, lam, sf, grad, nhatf_out, nhatfv_out=None):
        """the face unit interface normal flux on the internal faces in one face pass (mi_interface_nhatf): sf [x, y, z] face arrays, grad the
        cell gradient of alpha [gx, gy, gz], nhatfv_out three face arrays for the normal itself or None"""
        _chk(lib().mi_interface_nhatf(self.addr.h, C.c_double(delta_n), _ptr(lam), _ptrs(sf, 3), _ptrs(grad, 3), _ptr(nhatf_out), _ptrs(nhatfv_out, 3)))

    def interface_curvature(self, interface, nhatf, vol, K_out, b_nhatf=None):
        """K = -fvc::div(nHatf) over an Interface handle of this addressing (mi_interface_curvature)"""
        interface.curvature(nhatf, vol, K_out, b_nhatf)

    def surface_tension_force(self, sigma, lam, delta_coeffs, K, alpha, out, sngrad_corr=None):
        """fvc::interpolate(sigma*K)*fvc::snGrad(alpha) on the internal faces in one face pass (mi_surface_tension_force); sngrad_corr the
        explicit part of a corrected / limited snGrad or None"""
        _chk(lib().mi_surface_tension_force(self.addr.h, C.c_double(sigma), _ptr(lam), _ptr(delta_coeffs), _ptr(K), _ptr(alpha), _ptr(sngrad_corr), _ptr(out)))

    def near_interface(self, alpha, out):
        """out = pos(alpha - 0.01)*pos(0.99 - alpha) (mi_near_interface)"""
        n = (alpha if alpha is not None else out).numel()
        _chk(lib().mi_near_interface(self.addr.ctx.h, C.c_int64(n), _ptr(alpha), _ptr(out)))

    def min_max(self, x):
        """-> (min, max) of a device array on the host (mi_min_max); an empty array gives (+inf, -inf)"""
        lo, hi = C.c_double(0.0), C.c_double(0.0)
        _chk(lib().mi_min_max(self.addr.ctx.h, C.c_int64(0 if x is None else x.numel()), _ptr(x), C.byref(lo), C.byref(hi)))
        return float(lo.value), float(hi.value)

    def vec_max_value(self, x, value, out):
        """out = max(x, value), out may be x (mi_vec_max_value): the boundary line of bound"""
        n = (x if x is not None else out).numel()
        _chk(lib().mi_vec_max_value(self.addr.ctx.h, C.c_int64(n), _ptr(x), C.c_double(value), _ptr(out)))

    def fvc_average(self, average, mag_sf, ssf, out, b_mag_sf=None, b_ssf=None):
        """fvc::average(ssf) over an Average handle of this addressing (mi_fvc_average)"""
        average.fvc_average(mag_sf, ssf, out, b_mag_sf, b_ssf)

    def bound(self, average, lower_bound, lam, mag_sf, vsf_inout, b_mag_sf=None, b_face=None):
        """bound.C:45-54 on the internal field over an Average handle of this addressing (mi_bound)"""
        average.bound(lower_bound, lam, mag_sf, vsf_inout, b_mag_sf, b_face)

    def ke_production(self, nut, grad, g_out):
        """G = (nut*2)*magSqr(symm(gradU)) in one cell pass (mi_ke_production): grad the nine cell arrays d(U_j)/dx_k at 3*j + k"""
        pv = None if grad is None else (C.c_void_p * 9)(*[_ptr(x) for x in grad])
        n = (nut if nut is not None else g_out).numel()
        _chk(lib().mi_ke_production(self.addr.ctx.h, C.c_int64(n), _ptr(nut), pv, _ptr(g_out)))

    def ke_wall_cells(self, ke, coeffs, k, u, b_uw, b_delta_coeffs, b_y, b_nuw, b_nutw, g_inout, eps_inout, b_eps_out, b_pow_out=None):
        """the epsilon wall function on every wall patch over a KEpsilon handle of this addressing (mi_ke_wall_cells)"""
        ke.wall_cells(coeffs, k, u, b_uw, b_delta_coeffs, b_y, b_nuw, b_nutw, g_inout, eps_inout, b_eps_out, b_pow_out)

    def ke_epsilon_terms(self, coeffs, g, eps, k, nut, nu, su_out, sp_out, deps_out):
        """su = C1*G*eps/k, sp = C2*eps/k, deps = nut/sigmaEps + nu in one cell pass (mi_ke_epsilon_terms); nu a cell array or a number"""
        nu_dev, nu_value = (None, float(nu)) if isinstance(nu, (int, float)) else (nu, 0.0)
        n = (k if k is not None else su_out).numel()
        _chk(lib().mi_ke_epsilon_terms(self.addr.ctx.h, C.c_int64(n), C.byref(coeffs) if coeffs is not None else None, _ptr(g), _ptr(eps), _ptr(k),
                                       _ptr(nut), _ptr(nu_dev), C.c_double(nu_value), _ptr(su_out), _ptr(sp_out), _ptr(deps_out)))

    def ke_k_terms(self, eps, k, nut, nu, sp_out, dk_out):
        """sp = eps/k, dk = nut + nu in one cell pass (mi_ke_k_terms); nu a cell array or a number"""
        nu_dev, nu_value = (None, float(nu)) if isinstance(nu, (int, float)) else (nu, 0.0)
        n = (k if k is not None else sp_out).numel()
        _chk(lib().mi_ke_k_terms(self.addr.ctx.h, C.c_int64(n), _ptr(eps), _ptr(k), _ptr(nut), _ptr(nu_dev), C.c_double(nu_value), _ptr(sp_out), _ptr(dk_out)))

    def ke_nut(self, Cmu, k, eps, nut_out):
        """nut = Cmu*sqr(k)/eps (mi_ke_nut)"""
        n = (k if k is not None else nut_out).numel()
        _chk(lib().mi_ke_nut(self.addr.ctx.h, C.c_int64(n), C.c_double(Cmu), _ptr(k), _ptr(eps), _ptr(nut_out)))

    def ke_nut_wall(self, ke, coeffs, k, b_y, b_nuw, b_nutw_out, b_log_out=None):
        """nutkWallFunction on every wall face over a KEpsilon handle of this addressing (mi_ke_nut_wall)"""
        ke.nut_wall(coeffs, k, b_y, b_nuw, b_nutw_out, b_log_out)

    def les_simple_filter(self, average, lam, mag_sf, vf, out, b_mag_sf=None, b_face=None, n_cmpt=None):
        """the simple filter of up to nine components over an Average handle of this addressing (mi_les_simple_filter)"""
        average.les_simple_filter(lam, mag_sf, vf, out, b_mag_sf, b_face, n_cmpt)

    def _les_n(self, *xs):
        for x in xs:
            if x is not None and not isinstance(x, (list, tuple)):
                return x.numel()
        for x in xs:
            if isinstance(x, (list, tuple)):
                for y in x:
                    if y is not None:
                        return y.numel()
        return 0

    def les_delta_cube_root_vol(self, delta_coeff, thickness, vol, out, pow_out=None):
        """delta = deltaCoeff*pow(V, 1/3), or deltaCoeff*sqrt(V/thickness) with thickness > 0 (mi_les_delta_cube_root_vol)"""
        _chk(lib().mi_les_delta_cube_root_vol(self.addr.ctx.h, C.c_int64(self._les_n(vol, out)), C.c_double(delta_coeff), C.c_double(thickness), _ptr(vol),
                                              _ptr(out), _ptr(pow_out)))

    def les_smagorinsky(self, coeffs, delta, grad, nusgs_out, k_out=None):
        """Smagorinsky's k = (2ck/ce)*sqr(delta)*magSqr(dev(symm(gradU))) and nuSgs = ck*delta*sqrt(k) in one cell pass (mi_les_smagorinsky)"""
        _chk(lib().mi_les_smagorinsky(self.addr.ctx.h, C.c_int64(self._les_n(delta, nusgs_out)), C.byref(coeffs) if coeffs is not None else None, _ptr(delta),
                                      _ptrs(grad, 9), _ptr(k_out), _ptr(nusgs_out)))

    def les_k_terms(self, ce, nusgs, grad, k, delta, nu, g_out, sp_out, dk_out):
        """G = 2*nuSgs*magSqr(symm(gradU)), sp = ce*sqrt(k)/delta, dk = nuSgs + nu in one cell pass (mi_les_k_terms); ce and nu numbers or cell arrays"""
        ce_dev, ce_value = (None, float(ce)) if isinstance(ce, (int, float)) else (ce, 0.0)
        nu_dev, nu_value = (None, float(nu)) if isinstance(nu, (int, float)) else (nu, 0.0)
        _chk(lib().mi_les_k_terms(self.addr.ctx.h, C.c_int64(self._les_n(k, nusgs, g_out)), C.c_double(ce_value), _ptr(ce_dev), _ptr(nusgs), _ptrs(grad, 9),
                                  _ptr(k), _ptr(delta), _ptr(nu_dev), C.c_double(nu_value), _ptr(g_out), _ptr(sp_out), _ptr(dk_out)))

    def les_nusgs(self, ck, k, delta, out):
        """nuSgs = ck*sqrt(k)*delta (mi_les_nusgs); ck a number or a cell array"""
        ck_dev, ck_value = (None, float(ck)) if isinstance(ck, (int, float)) else (ck, 0.0)
        _chk(lib().mi_les_nusgs(self.addr.ctx.h, C.c_int64(self._les_n(k, delta, out)), C.c_double(ck_value), _ptr(ck_dev), _ptr(k), _ptr(delta), _ptr(out)))

    def les_dyn_moments(self, u, grad, sqr_u_out, magsqr_u_out, d_out, magsqr_d_out):
        """sqr(U), magSqr(U), D = symm(gradU) and magSqr(D) in one cell pass (mi_les_dyn_moments)"""
        _chk(lib().mi_les_dyn_moments(self.addr.ctx.h, C.c_int64(self._les_n(magsqr_u_out, magsqr_d_out, u)), _ptrs(u, 3), _ptrs(grad, 9), _ptrs(sqr_u_out, 6),
                                      _ptr(magsqr_u_out), _ptrs(d_out, 6), _ptr(magsqr_d_out)))

    def les_dyn_level1(self, clip, delta, nueff, f_u, f_sqr_u, f_magsqr_u, f_d, f_magsqr_d, kk_out, ll_out, mm_out, ce_num_out, ce_den_out, pow_out=None):
        """KK, LL, MM and the two fields of ce between the first and the second filter level (mi_les_dyn_level1)"""
        _chk(lib().mi_les_dyn_level1(self.addr.ctx.h, C.c_int64(self._les_n(delta, nueff, kk_out)), C.c_int(1 if clip else 0), _ptr(delta), _ptr(nueff),
                                     _ptrs(f_u, 3), _ptrs(f_sqr_u, 6), _ptr(f_magsqr_u), _ptrs(f_d, 6), _ptr(f_magsqr_d), _ptr(kk_out), _ptrs(ll_out, 6),
                                     _ptrs(mm_out, 6), _ptr(ce_num_out), _ptr(ce_den_out), _ptr(pow_out)))

    def les_dyn_level2(self, f_ll, f_mm, lm_out, mmmm_out):
        """lm = 0.5*(fLL && fMM), mmmm = magSqr(fMM) (mi_les_dyn_level2)"""
        _chk(lib().mi_les_dyn_level2(self.addr.ctx.h, C.c_int64(self._les_n(lm_out, mmmm_out, f_ll)), _ptrs(f_ll, 6), _ptrs(f_mm, 6), _ptr(lm_out), _ptr(mmmm_out)))

    def les_dyn_coeffs(self, f_lm, f_mmmm, f_ce_num, f_ce_den, ck_out, ce_out):
        """ck = 0.5*(mag(c) + c) with c = f_lm/(f_mmmm + VSMALL); ce likewise from f_ce_num/f_ce_den (mi_les_dyn_coeffs)"""
        _chk(lib().mi_les_dyn_coeffs(self.addr.ctx.h, C.c_int64(self._les_n(f_lm, ck_out)), _ptr(f_lm), _ptr(f_mmmm), _ptr(f_ce_num), _ptr(f_ce_den),
                                     _ptr(ck_out), _ptr(ce_out)))

    def sst_production(self, nut, grad, s2_out, g_out, mag_out=None):
        """S2 = 2*magSqr(symm(gradU)), G = nut*S2 and optionally mag(symm(gradU)) in one cell pass (mi_sst_production): grad as ke_production's"""
        pv = None if grad is None else (C.c_void_p * 9)(*[_ptr(x) for x in grad])
        n = (nut if nut is not None else g_out).numel()
        _chk(lib().mi_sst_production(self.addr.ctx.h, C.c_int64(n), _ptr(nut), pv, _ptr(s2_out), _ptr(g_out), _ptr(mag_out)))

    def sst_wall_cells(self, ke, coeffs, k, u, b_uw, b_delta_coeffs, b_y, b_nuw, b_nutw, g_inout, omega_inout, b_omega_out):
        """the omega wall function on every wall patch over a KEpsilon handle of this addressing (mi_sst_wall_cells)"""
        ke.sst_wall_cells(coeffs, k, u, b_uw, b_delta_coeffs, b_y, b_nuw, b_nutw, g_inout, omega_inout, b_omega_out)

    def sst_blend(self, coeffs, f3, grad_k, grad_omega, k, omega, y, nut, s2, nu, f1_out, su_out, sp_out, susp_out, domega_out, dk_out,
                  cdkomega_out=None, arg1_out=None, f23_out=None, tanh3_out=None):
        """CDkOmega, F1, F23, the blended coefficients, the omega equation's su / sp / susp, DomegaEff and DkEff in one cell pass
        (mi_sst_blend); nu a cell array or a number; f3 the model's F3 switch"""
        x = SstBlendArrays()
        for d in range(3):
            x.grad_k_dev[d] = _ptr(None if grad_k is None else grad_k[d]).value
            x.grad_omega_dev[d] = _ptr(None if grad_omega is None else grad_omega[d]).value
        nu_dev, x.nu_value = (None, float(nu)) if isinstance(nu, (int, float)) else (nu, 0.0)
        x.k_dev, x.omega_dev, x.y_dev, x.nut_dev, x.s2_dev, x.nu_dev_or_null = (_ptr(t).value for t in (k, omega, y, nut, s2, nu_dev))
        x.f1_out_dev, x.su_out_dev, x.sp_out_dev, x.susp_out_dev, x.domega_out_dev, x.dk_out_dev = \
            (_ptr(t).value for t in (f1_out, su_out, sp_out, susp_out, domega_out, dk_out))
        x.cdkomega_out_dev_or_null, x.arg1_out_dev_or_null, x.f23_out_dev_or_null, x.tanh3_out_dev_or_null = \
            (_ptr(t).value for t in (cdkomega_out, arg1_out, f23_out, tanh3_out))
        n = (k if k is not None else f1_out).numel()
        _chk(lib().mi_sst_blend(self.addr.ctx.h, C.c_int64(n), C.byref(coeffs) if coeffs is not None else None, C.c_int(int(bool(f3))), C.byref(x)))

    def sst_omega_sources(self, vol, su, sp, susp, omega, diag_inout, source_inout):
        """the omega equation's == su - fvm::Sp(sp, omega) - fvm::SuSp(susp, omega) in the reference's grouping, in place on the assembled
        diagonal and source (mi_sst_omega_sources)"""
        n = (omega if omega is not None else diag_inout).numel()
        _chk(lib().mi_sst_omega_sources(self.addr.ctx.h, C.c_int64(n), _ptr(vol), _ptr(su), _ptr(sp), _ptr(susp), _ptr(omega), _ptr(diag_inout),
                                        _ptr(source_inout)))

    def sst_k_terms(self, coeffs, g, k, omega, su_out, sp_out):
        """su = min(G, c1*betaStar*k*omega), sp = betaStar*omega in one cell pass (mi_sst_k_terms)"""
        n = (k if k is not None else su_out).numel()
        _chk(lib().mi_sst_k_terms(self.addr.ctx.h, C.c_int64(n), C.byref(coeffs) if coeffs is not None else None, _ptr(g), _ptr(k), _ptr(omega),
                                  _ptr(su_out), _ptr(sp_out)))

    def sst_nut(self, coeffs, f3, k, omega, y, s, nu, nut_out, f23_out=None, constructor_form=False):
        """nut = a1*k/max(a1*omega, b1*F23*sqrt(S2)) with F23 recomputed in the pass (mi_sst_nut); constructor_form: s is mag(symm(gradU)) and
        the strain term b1*F23*sqrt(2.0)*s; nu a cell array or a number"""
        nu_dev, nu_value = (None, float(nu)) if isinstance(nu, (int, float)) else (nu, 0.0)
        n = (k if k is not None else nut_out).numel()
        _chk(lib().mi_sst_nut(self.addr.ctx.h, C.c_int64(n), C.byref(coeffs) if coeffs is not None else None, C.c_int(int(bool(f3))),
                              C.c_int(int(bool(constructor_form))), _ptr(k), _ptr(omega), _ptr(y), _ptr(s), _ptr(nu_dev), C.c_double(nu_value),
                              _ptr(nut_out), _ptr(f23_out)))

    def sa_terms(self, coeffs, kind, ashford, nutilda, grad, grad_nutilda, y, nu, su_grad_out, su_prod_out, sp_out, dnu_out, fv1_out, delta=None,
                 nusgs=None, hmax=None, **optional):
        """The Spalart-Allmaras model's cell pass (mi_sa_terms): kind "RAS" | "DES" | "DDES" | "IDDES" (or MI_SA_*), ashford the ashfordCorrection
        switch; nu a cell array or a number; delta for the DES kinds, nusgs for DDES and IDDES, hmax for IDDES; optional outputs by the names
        of SA_OPTIONAL"""
        unknown = set(optional) - set(SA_OPTIONAL)
        if unknown:
            raise TypeError("sa_terms: unknown output " + ", ".join(sorted(unknown)))
        x = SaCells()
        x.nutilda_dev = _ptr(nutilda).value
        for i in range(9):
            x.grad_dev[i] = _ptr(None if grad is None else grad[i]).value
        for i in range(3):
            x.grad_nutilda_dev[i] = _ptr(None if grad_nutilda is None else grad_nutilda[i]).value
        nu_dev, x.nu_value = (None, float(nu)) if isinstance(nu, (int, float)) else (nu, 0.0)
        x.y_dev, x.nu_dev_or_null, x.delta_dev, x.nusgs_dev, x.hmax_dev = (_ptr(t).value for t in (y, nu_dev, delta, nusgs, hmax))
        x.su_grad_out_dev, x.su_prod_out_dev, x.sp_out_dev, x.dnu_out_dev, x.fv1_out_dev = \
            (_ptr(t).value for t in (su_grad_out, su_prod_out, sp_out, dnu_out, fv1_out))
        for name in SA_OPTIONAL:
            setattr(x, name + "_out_dev_or_null", _ptr(optional.get(name)).value)
        n = self._les_n(nutilda, y, fv1_out)
        _chk(lib().mi_sa_terms(self.addr.ctx.h, C.c_int64(n), C.byref(coeffs) if coeffs is not None else None, C.c_int(SA_KINDS.get(kind, kind)),
                               C.c_int(int(bool(ashford))), C.byref(x)))

    def sa_nut(self, coeffs, nutilda, nut_out, fv1=None, nu=None, fv1_out=None):
        """nut = fv1*nuTilda (mi_sa_nut): with fv1 the array sa_terms wrote before the solve (the RAS correct()), or with nu (a cell array or a
        number) fv1 recomputed from nuTilda, as updateSubGridScaleFields() of the LES classes does"""
        recompute = fv1 is None
        nu_dev, nu_value = (None, float(nu)) if isinstance(nu, (int, float)) else (nu, 0.0)
        _chk(lib().mi_sa_nut(self.addr.ctx.h, C.c_int64(self._les_n(nutilda, nut_out)), C.byref(coeffs) if coeffs is not None else None,
                             C.c_int(int(recompute)), _ptr(nutilda), _ptr(fv1), _ptr(nu_dev), C.c_double(nu_value), _ptr(nut_out), _ptr(fv1_out)))

    def sa_nut_spalding_wall(self, ke, coeffs, u, b_uw, b_delta_coeffs, b_y, b_nuw, b_nutw_inout, b_exp_out=None, b_iter_out=None):
        """nutUSpaldingWallFunction on every wall face over a KEpsilon handle of this addressing (mi_sa_nut_spalding_wall)"""
        ke.sa_nut_spalding_wall(coeffs, u, b_uw, b_delta_coeffs, b_y, b_nuw, b_nutw_inout, b_exp_out, b_iter_out)

    def thermo_calculate(self, model, he, p, t0, t_out, psi_out, mu_out, alpha_out, rho_out=None, rho_form=0, iters_out=None):
        """T = THE(he, p, t0) by the reference's Newton iteration, then psi, mu, alpha and (rho_form 1: p/(R*T), 2: psi*p) rho at the new T in one
        cell pass (mi_thermo_calculate); t_out may be t0 or he; iters_out an int32 tensor for the evaluation counts or None"""
        n = (he if he is not None else t_out).numel()
        it = None
        if iters_out is not None:
            assert iters_out.is_contiguous() and iters_out.element_size() == 4
            it = C.c_void_p(iters_out.data_ptr())
        _chk(lib().mi_thermo_calculate(self.addr.ctx.h, C.byref(model) if model is not None else None, C.c_int(int(rho_form)), C.c_int64(n), _ptr(he),
                                       _ptr(p), _ptr(t0), _ptr(t_out), _ptr(psi_out), _ptr(mu_out), _ptr(alpha_out), _ptr(rho_out), it))

    def thermo_calculate_boundary(self, boundary, model, patch_kind, b_he, b_p, b_t, b_psi_out, b_mu_out, b_alpha_out, b_rho_out=None, rho_form=0,
                                  b_t_out=None):
        """the patch loop of hePsiThermo / heRhoThermo ::calculate() on every patch in one launch (mi_thermo_calculate_boundary): patch_kind per
        patch 0 skip, 1 fixesValue (b_he = HE(p, T)), 2 otherwise (T = THE(he, p, T)); the new temperature of kind 2 goes to b_t_out, b_t itself
        when None (OpenFOAM's meaning; b_t_out=b_he is the reference's transform)"""
        pk = None if patch_kind is None else (C.c_int32 * max(len(patch_kind), 1))(*[int(k) for k in patch_kind])
        _chk(lib().mi_thermo_calculate_boundary(self.addr.h, boundary.h if boundary is not None else None, C.byref(model) if model is not None else None,
                                                pk, C.c_int(int(rho_form)), _ptr(b_he), _ptr(b_p), _ptr(b_t), _ptr(b_t if b_t_out is None else b_t_out),
                                                _ptr(b_psi_out), _ptr(b_mu_out), _ptr(b_alpha_out), _ptr(b_rho_out)))

    def thermo_he(self, model, p, t, he_out):
        """he = HE(p, T) (mi_thermo_he): heThermo::init on the cells, or on a patch's slice of the boundary arrays"""
        n = (p if p is not None else he_out).numel()
        _chk(lib().mi_thermo_he(self.addr.ctx.h, C.byref(model) if model is not None else None, C.c_int64(n), _ptr(p), _ptr(t), _ptr(he_out)))

    def thermo_property(self, model, kind, p, t, out):
        """one of Cp, Cv, gamma, Cpv, CpByCpv, kappa (THERMO_PROPERTIES) from p and T (mi_thermo_property), cells or a patch slice"""
        n = (p if p is not None else out).numel()
        k = THERMO_PROPERTIES[kind] if isinstance(kind, str) else int(kind)
        _chk(lib().mi_thermo_property(self.addr.ctx.h, C.byref(model) if model is not None else None, C.c_int(k), C.c_int64(n), _ptr(p), _ptr(t), _ptr(out)))

    def central_flux(self, scheme, cd_weights, sf, mag_sf, cells, c, out):
        """rhoCentralFoam.C:62-185 on the internal faces in one face pass (mi_central_flux): scheme a CentralScheme (central_scheme), sf
        [x, y, z] face arrays, cells a CentralCells (central_cells), c the cell centres [x, y, z], out a CentralOut (central_out)"""
        _chk(lib().mi_central_flux(self.addr.h, C.byref(scheme) if scheme is not None else None, _ptr(cd_weights), _ptrs(sf, 3), _ptr(mag_sf),
                                   C.byref(cells) if cells is not None else None, _ptrs(c, 3), C.byref(out) if out is not None else None))

    def central_sound_speed(self, cp, cv, psi, rpsi_out, c_out):
        """rPsi = 1.0/psi and c = sqrt((Cp/Cv)*rPsi) in one cell pass (mi_central_sound_speed)"""
        n = (psi if psi is not None else rpsi_out).numel()
        _chk(lib().mi_central_sound_speed(self.addr.ctx.h, C.c_int64(n), _ptr(cp), _ptr(cv), _ptr(psi), _ptr(rpsi_out), _ptr(c_out)))

    def vec_div(self, x, y, out):
        """out = x/y element by element, out may alias either (mi_vec_div)"""
        _chk(lib().mi_vec_div(self.addr.ctx.h, C.c_int64(x.numel()), _ptr(x), _ptr(y), _ptr(out)))

    def central_courant(self, delta_coeffs, mag_sf, amaxsf, b_delta_coeffs=None, b_mag_sf=None, b_amaxsf=None):
        """-> (max over internal and boundary faces of (deltaCoeffs*amaxSf)/magSf, sum over the internal faces of deltaCoeffs*amaxSf) on the
        host (mi_central_courant, compressibleCourantNo.H:35-47); a mesh without internal faces gives (0.0, 0.0)"""
        mx, sm = C.c_double(0.0), C.c_double(0.0)
        nb = 0 if b_amaxsf is None else b_amaxsf.numel()
        _chk(lib().mi_central_courant(self.addr.h, _ptr(delta_coeffs), _ptr(mag_sf), _ptr(amaxsf), C.c_int64(nb), _ptr(b_delta_coeffs), _ptr(b_mag_sf),
                                      _ptr(b_amaxsf), C.byref(mx), C.byref(sm)))
        return float(mx.value), float(sm.value)

    def vec_min(self, x, y, out):
        """out = min(x, y) element by element, out may alias either (mi_vec_min): minOp over the two sides of a cyclic pair"""
        _chk(lib().mi_vec_min(self.addr.ctx.h, C.c_int64(x.numel()), _ptr(x), _ptr(y), _ptr(out)))

    def lust_weights(self, cd_weights, face_flux, w_out):
        """LUST weights 0.75*cd_weights + 0.25*pos(faceFlux) (LUST.H:104-110)"""
        _chk(lib().mi_lust_weights(self.addr.ctx.h, C.c_int64(face_flux.numel()), _ptr(cd_weights), _ptr(face_flux), _ptr(w_out)))

    def submul(self, x, y, inout):
        """inout -= x*y (source -= V*div(...))"""
        _chk(lib().mi_vec_submul(self.addr.ctx.h, C.c_int64(inout.numel()), _ptr(x), _ptr(y), _ptr(inout)))

    def axpby(self, a, x, b, y, out):
        _chk(lib().mi_vec_axpby(self.addr.ctx.h, C.c_int64(x.numel()), C.c_double(a), _ptr(x), C.c_double(b), _ptr(y), _ptr(out)))

    def assemble(self, upper_out, diag_out, lower_out=None, sources_out=(), ddt=None, div=None, laplacian=None, sp=None, su=(), sum_mag_out=None):
        """[fvm::ddt] + [fvm::div] - [fvm::laplacian] [+- fvm::Sp] [+- su] in one row pass (mi_fvm_assemble).
        ddt = dict(r_delta_t=, vol=, psi_old=[...], rho=None | tensor, rho_old=None | tensor, rho_value=1.0); div = dict(flux=, weights=None (upwind) | tensor);
        laplacian = dict(delta_coeffs=, gamma_magsf=); sp = (field, sign); su = [(sign, [field per rhs]), ...]; vol is taken from ddt or the `vol` key of sp / su
        through ddt["vol"] (pass ddt=dict(vol=...) with r_delta_t omitted for no time derivative).
        div["correction"] = dict(scale=1.0 | 0.25, cf=[x, y, z], c=[x, y, z], grad=[[gx, gy, gz] per rhs]): the explicit correction of linearUpwind / LUST
        in the same pass (mi_fvm_assemble_corrected).
        ddt["backward"] = dict(coeffs=ddt_backward_coeffs(...), psi_old_old=[...], rho_old_old=None | tensor): the backward time derivative in place of
        Euler's (mi_fvm_assemble_backward), with or without the correction.
        ddt["crank_nicolson"] = dict(oc=, ddt0=[...]): the CrankNicolson time derivative (mi_fvm_assemble_cn); r_delta_t carries rDtCoef and the ddt0
        fields are already updated for this time step.  Not together with "backward".
        ddt["local"] = dict(r_delta_t=tensor): the localEuler / CoEuler time derivative, rDeltaT a cell field (mi_fvm_assemble_local; the scalar r_delta_t is
        ignored).  Not together with "backward" or "crank_nicolson".
        div["bounded"] = tensor: bounded Gauss convection, the tensor fvc::surfaceIntegrate(faceFlux) with the boundary faces (mi_fvm_assemble_local); with
        ddt["local"], with Euler, or with no time derivative (steadyState)."""
        t = FvmTerms()
        n_rhs = len(sources_out)
        keep = []
        if ddt is not None and ("r_delta_t" in ddt or "local" in ddt):
            t.ddt = 1; t.r_delta_t = float(ddt.get("r_delta_t", 0.0)); t.rho_value = float(ddt.get("rho_value", 1.0))
            t.rho_dev = _ptr(ddt.get("rho")).value; t.rho_old_dev = _ptr(ddt.get("rho_old")).value
            po = (C.c_void_p * max(n_rhs, 1))(*[_ptr(x) for x in ddt["psi_old"]]); keep.append(po)
            t.psi_old_dev = C.cast(po, C.POINTER(C.c_void_p))
        if ddt is not None:
            t.vol_dev = _ptr(ddt.get("vol")).value
        if div is not None:
            t.div_flux_dev = _ptr(div["flux"]).value; t.div_weights_dev = _ptr(div.get("weights")).value
        if laplacian is not None:
            t.lap_delta_coeffs_dev = _ptr(laplacian["delta_coeffs"]).value; t.lap_gamma_magsf_dev = _ptr(laplacian["gamma_magsf"]).value
        if sp is not None:
            t.sp_dev = _ptr(sp[0]).value; t.sp_sign = float(sp[1])
        t.n_rhs = n_rhs; t.n_su = len(su)
        if su:
            sd = (C.c_void_p * (len(su) * n_rhs))(*[_ptr(f) for _, fields in su for f in fields]); keep.append(sd)
            sg = (C.c_double * len(su))(*[float(sign) for sign, _ in su]); keep.append(sg)
            t.su_dev = C.cast(sd, C.POINTER(C.c_void_p)); t.su_sign = C.cast(sg, C.POINTER(C.c_double))
        so = (C.c_void_p * max(n_rhs, 1))(*[_ptr(x) for x in sources_out])
        corr = (div or {}).get("correction")
        back = (ddt or {}).get("backward")
        cn = (ddt or {}).get("crank_nicolson")
        local = (ddt or {}).get("local")
        bounded = (div or {}).get("bounded")
        if back is not None and cn is not None:
            raise MiError("Assembly.assemble: ddt takes 'backward' or 'crank_nicolson', not both")
        if (local is not None or bounded is not None) and (back is not None or cn is not None):
            raise MiError("Assembly.assemble: ddt['local'] and div['bounded'] do not combine with 'backward' or 'crank_nicolson'")
        if local is not None or bounded is not None:
            b = FvmLocalTerms()
            b.r_delta_t_dev = _ptr(None if local is None else local["r_delta_t"]).value
            b.div_flux_dev = _ptr(bounded).value
            entry, form = lib().mi_fvm_assemble_local, (C.byref(b),)
        elif cn is not None:
            b = DdtCnTerms()
            b.oc = float(cn["oc"])
            d0 = (C.c_void_p * max(n_rhs, 1))(*[_ptr(x) for x in cn["ddt0"]]); keep.append(d0)
            b.ddt0_dev = C.cast(d0, C.POINTER(C.c_void_p))
            entry, form = lib().mi_fvm_assemble_cn, (C.byref(b),)
        elif back is not None:
            b = DdtBackward()
            b.coefft, b.coefft0, b.coefft00 = [float(x) for x in back["coeffs"]]
            b.rho_old_old_dev = _ptr(back.get("rho_old_old")).value
            poo = (C.c_void_p * max(n_rhs, 1))(*[_ptr(x) for x in back["psi_old_old"]]); keep.append(poo)
            b.psi_old_old_dev = C.cast(poo, C.POINTER(C.c_void_p))
            entry, form = lib().mi_fvm_assemble_backward, (C.byref(b),)
        else:
            entry, form = lib().mi_fvm_assemble_corrected, ()      # without a correction: mi_fvm_assemble
        k = None if corr is None else div_correction(corr["cf"], corr["c"], corr["grad"], corr.get("scale", 1.0))
        _chk(entry(self.addr.h, C.byref(t), *form, None if k is None else C.byref(k), _ptr(lower_out), _ptr(upper_out), _ptr(diag_out), so, _ptr(sum_mag_out)))

    def fvc_div(self, face_flux, weights, vf, vol, face_out, div_out):
        """fvc::div(faceFlux, vf) (gaussConvectionScheme.C:117-140); weights None: upwind"""
        _chk(lib().mi_fvc_div(self.addr.h, _ptr(face_flux), _ptr(weights), _ptr(vf), _ptr(vol), _ptr(face_out), _ptr(div_out)))

    def set_reference(self, celli, value, diag, source):
        """fvMatrix::setReference (fvMatrix.C:964-981)"""
        _chk(lib().mi_fvm_set_reference(self.addr.h, C.c_int32(celli), C.c_double(value), _ptr(diag), _ptr(source)))

    def set_values(self, cell_labels, values, psi, diag, source, upper_in, lower_in, upper_out, lower_out, patches=(), internal_coeffs=(), boundary_coeffs=(),
                   upstream=False):
        """fvMatrix::setValues (fvMatrix.C:454-656); cell_labels: int32 device tensor"""
        n = len(patches)
        ph = (C.c_void_p * max(n, 1))(*[p.h for p in patches])
        ic = (C.c_void_p * max(n, 1))(*[_ptr(t) for t in internal_coeffs])
        bc = (C.c_void_p * max(n, 1))(*[_ptr(t) for t in boundary_coeffs])
        assert cell_labels.is_contiguous() and cell_labels.element_size() == 4
        _chk(lib().mi_fvm_set_values(self.addr.h, C.c_int32(cell_labels.numel()), C.c_void_p(cell_labels.data_ptr()), _ptr(values), C.c_int32(int(upstream)),
                                     _ptr(psi), _ptr(diag), _ptr(source), _ptr(upper_in), _ptr(lower_in), _ptr(upper_out), _ptr(lower_out),
                                     C.c_int32(n), ph, ic, bc))

    def relax_multi(self, alpha, diag, lower, upper, sources, psis, sum_mag=None, patches=(), internal_coeffs=(), boundary_coeffs=(), coupled=()):
        """fvMatrix<Type>::relax for n_rhs components sharing the diagonal; sum_mag: mi_fvm_assemble's sumMagOffDiag by-product (completed in place)"""
        n = len(patches)
        ph = (C.c_void_p * max(n, 1))(*[p.h for p in patches])
        ic = (C.c_void_p * max(n, 1))(*[_ptr(t) for t in internal_coeffs])
        bc = (C.c_void_p * max(n, 1))(*[_ptr(t) for t in boundary_coeffs])
        cp = (C.c_int32 * max(n, 1))(*[int(v) for v in coupled])
        m = len(sources)
        sp = (C.c_void_p * max(m, 1))(*[_ptr(t) for t in sources])
        pp = (C.c_void_p * max(m, 1))(*[_ptr(t) for t in psis])
        _chk(lib().mi_relax_multi(self.addr.h, C.c_double(alpha), _ptr(diag), _ptr(lower), _ptr(upper), _ptr(sum_mag), C.c_int32(m), sp, pp,
                                  C.c_int32(n), ph, ic, bc, cp))

    def relax(self, alpha, diag, lower, upper, source, psi, patches=(), internal_coeffs=(), boundary_coeffs=(), coupled=()):
        n = len(patches)
        ph = (C.c_void_p * max(n, 1))(*[p.h for p in patches])
        ic = (C.c_void_p * max(n, 1))(*[_ptr(t) for t in internal_coeffs])
        bc = (C.c_void_p * max(n, 1))(*[_ptr(t) for t in boundary_coeffs])
        cp = (C.c_int32 * max(n, 1))(*[int(v) for v in coupled])
        _chk(lib().mi_relax(self.addr.h, C.c_double(alpha), _ptr(diag), _ptr(lower), _ptr(upper), _ptr(source), _ptr(psi),
                            C.c_int32(n), ph, ic, bc, cp))
