"""ctypes binding of libisph_hip.so (include/isph_hip.h) -- the product path.

Nothing in here touches the oracle or any CPU fallback: if the HIP library is
missing or no GPU is usable, calls raise.  Arrays may be numpy (host) or torch
CUDA tensors (device pointers are passed straight through).
"""
import ctypes as C
import sys
import os

import numpy as np

from . import build as _build

UID_BYTES = 128
NOT_SINGULAR, NULLSPACE, PINZERO, DOUBLEDIAG = 0, 1, 2, 3
KERNELS = {"wendland": 0, "quintic": 1, "cubic": 2}

EXPORTS = [
    "isph_ctx_create", "isph_comm_unique_id", "isph_ctx_create_dist", "isph_ctx_create_hostcomm", "isph_ctx_sync", "isph_ctx_destroy", "isph_pool_trim", "isph_pool_set_cap", "isph_set_exact_stream_threshold", "isph_pool_cached_bytes", "isph_pool_info", "isph_halo_create", "isph_halo_forward", "isph_halo_destroy", "isph_prec_create_overlap",
    "isph_last_error", "isph_mat_create_csr", "isph_mat_create_csr_bjacobi", "isph_mat_create_csr_blocks", "isph_mat_create_csr_coords", "isph_mat_create_csr_coords_bjacobi", "isph_ingress_info", "isph_mat_set_halo", "isph_mat_info", "isph_mat_export_csr", "isph_mat_export_rows", "isph_mat_column_bits",
    "isph_mat_destroy", "isph_spmv", "isph_spmv_time", "isph_prec_create", "isph_prec_create_blocks", "isph_prec_create_blocks_fill", "isph_prec_apply",
    "isph_prec_apply_multi", "isph_prec_multi_path",
    "isph_prec_export_ilu", "isph_prec_nnz", "isph_prec_info", "isph_prec_destroy", "isph_solver_params_default", "isph_solve",
    "isph_ctx_set_profile", "isph_ctx_hold_neighbours", "isph_ctx_profile_read", "isph_ctx_set_ordering", "isph_ctx_set_periodic_box", "isph_mat_ordering_info", "isph_mat_ordering", "isph_mat_ordering_faces", "isph_ctx_halo_profile_read", "isph_ctx_comm_info", "isph_device_identity", "isph_assemble_poisson", "isph_assemble_helmholtz", "isph_assemble_solute_transport", "isph_assemble_applied_potential", "isph_compute_volumes", "isph_compute_pnd", "isph_compute_corrections", "isph_gradient", "isph_divergence", "isph_correct_velocity_pressure",
    "isph_advance_begin", "isph_advance_end", "isph_compute_shift", "isph_apply_shift", "isph_shift_particles",
    "isph_solve_block", "isph_assemble_block_helmholtz", "isph_amg_params_default", "isph_prec_create_amg", "isph_prec_amg_levels", "isph_prec_amg_info",
    "isph_prec_amg_export", "isph_prec_amg_aggregates", "isph_prec_amg_path", "isph_prec_amg_refreshes", "isph_prec_amg_set_nullvec",
    "isph_schwarz_params_default", "isph_prec_create_schwarz", "isph_prec_schwarz_info", "isph_prec_schwarz_paths", "isph_prec_schwarz_timing", "isph_prec_schwarz_export",
    "isph_pb_params_default", "isph_assemble_poisson_boltzmann", "isph_pb_residual", "isph_pb_jacobian", "isph_solve_poisson_boltzmann",
    "isph_compute_normals", "isph_csf_params_default", "isph_csf_phase_normal", "isph_csf_force", "isph_surface_tension_csf", "isph_pairwise_force",
    "isph_smooth_field", "isph_ek_params_default", "isph_electrostatic_force", "isph_random_stress_tensor", "isph_random_stress_force",
    "isph_force_from_random_stress", "isph_cheb_params_default", "isph_prec_create_chebyshev", "isph_prec_value_bits", "isph_prec_cycle_bits",
    "isph_prec_eig_estimate",
    "isph_poly_params_default", "isph_prec_create_gmres_poly", "isph_prec_poly_info", "isph_prec_type_kind",
    "isph_ilu_params_default", "isph_prec_create_ilu",
    "isph_nlist_build", "isph_nlist_info", "isph_nlist_get", "isph_nlist_destroy",
    "isph_nlist_build_dist", "isph_nlist_dist_info", "isph_nlist_dist_get", "isph_nlist_forward", "isph_nlist_forward_int",
    "isph_migrate", "isph_migrated_info", "isph_migrated_get", "isph_migrated_destroy",
    "isph_ctx_hold_pattern", "isph_mat_update_values", "isph_mat_pattern_info", "isph_prec_refactor",
    "isph_recycle_create", "isph_recycle_destroy", "isph_recycle_reset", "isph_recycle_info", "isph_recycle_export", "isph_recycle_import",
    "isph_solve_recycle", "isph_dense_tall_gemm", "isph_dense_block_gram",
    "isph_ghost_fill", "isph_zero_mean_pressure", "isph_status", "isph_tgv_error",
    "isph_ins_params_default", "isph_ins_create", "isph_ins_destroy", "isph_ins_set_state", "isph_ins_set_list", "isph_ins_rebuild",
    "isph_ins_sizes", "isph_ins_get", "isph_ins_pre", "isph_ins_view", "isph_ins_force", "isph_ins_add_force", "isph_ins_solve",
    "isph_ins_advance", "isph_ins_shift", "isph_ins_diagnostics", "isph_ins_run",
    "isph_nlist_forward_multi", "isph_zero_mean_pressure_dist", "isph_status_dist", "isph_tgv_error_dist",
    "isph_ins_create_dist", "isph_ins_set_state_dist", "isph_ins_sizes_dist",
]


class AmgParams(C.Structure):
    """Mirror of isph_amg_params == the keys PrecondWrapper_ML::setParameters sets (precond_ml.h:44-55).  smoother: 0 / 1
    the Gauss-Seidel smoothers, 2 Chebyshev, 4 block ILU(ilu_fill) (ML's "IFPACK" smoother; ilu_fill = "fact: level-of-fill",
    0..8)."""
    _fields_ = [("max_levels", C.c_int), ("coarse_max", C.c_int), ("omega", C.c_double), ("block", C.c_int),
                ("sweeps", C.c_int), ("theta", C.c_double), ("smoother", C.c_int), ("cheb_ratio", C.c_double),
                ("cheb_value_bits", C.c_int), ("eig_type", C.c_int), ("eig_iters", C.c_int), ("cycle_bits", C.c_int),
                ("ilu_fill", C.c_int)]

    def __init__(self, **kw):
        super().__init__()
        lib().isph_amg_params_default(C.byref(self))
        for k, v in kw.items():
            setattr(self, k, v)


class SolverParams(C.Structure):
    """Mirror of isph_solver_params == SolverLin_Belos::setParameters keys
    (ref: solver_lin_belos.h:224-264)."""
    _fields_ = [("solver_type", C.c_int), ("flexible", C.c_int), ("num_blocks", C.c_int),
                ("max_iters", C.c_int), ("max_restarts", C.c_int), ("tol", C.c_double),
                ("ortho", C.c_int), ("verbose", C.c_int), ("num_recycled", C.c_int), ("basis_bits", C.c_int)]

    def __init__(self, solver_type=0, flexible=1, num_blocks=50, max_iters=500, max_restarts=15, tol=1e-8,
                 ortho=0, verbose=0, num_recycled=50, basis_bits=0):
        """solver_type 0 "Block GMRES", 1 "Block CG", 2 "Recycling GMRES" (GCRO-DR(num_blocks, num_recycled));
        basis_bits 0 / 64: the fp64 Krylov basis, 32: the basis stored in single precision (GMRES only, see
        include/isph_hip.h)"""
        super().__init__(solver_type, flexible, num_blocks, max_iters, max_restarts, tol, ortho, verbose, num_recycled,
                         basis_bits)


class PBParams(C.Structure):
    """Mirror of isph_pb_params: the Poisson-Boltzmann physics (kappa^2 = 2 ezcb / psiref, gamma, linearized) and the
    NOX list of SolverNOX_Stratimikos (solver_nox_impl.h:78-145, solver_nox_stratimikos.h:84-122).  Keyword arguments
    override the defaults of isph_pb_params_default; `amg` / `linear` may be given as AmgParams / SolverParams or as a
    dict of fields to change.  prec_refresh = 1: at prec_max_age the preconditioner is refreshed on the new Jacobian
    (isph_prec_refactor) instead of being destroyed and built again; PBInfo.prec_refreshes counts those."""
    _fields_ = [("kappasq", C.c_double), ("gamma", C.c_double), ("linearized", C.c_int), ("max_iters", C.c_int),
                ("f_tol", C.c_double), ("update_tol", C.c_double), ("prec_max_age", C.c_int), ("prec_kind", C.c_int),
                ("amg", AmgParams), ("linear", SolverParams), ("prec_refresh", C.c_int)]

    def __init__(self, **kw):
        super().__init__()
        lib().isph_pb_params_default(C.byref(self))
        for k, v in kw.items():
            if k in ("amg", "linear") and isinstance(v, dict):
                sub = getattr(self, k)
                for k2, v2 in v.items():
                    setattr(sub, k2, v2)
            else:
                setattr(self, k, v)


class PBInfo(C.Structure):
    """isph_pb_info: status 1 converged, 0 MaxIters, -1 non-finite ||F||"""
    _fields_ = [("status", C.c_int), ("newton_iters", C.c_int), ("linear_iters", C.c_int), ("prec_builds", C.c_int),
                ("norm_f", C.c_double), ("norm_update", C.c_double), ("ms", C.c_double), ("prec_refreshes", C.c_int)]


class SolveInfo(C.Structure):
    _fields_ = [("converged", C.c_int), ("iters", C.c_int), ("restarts", C.c_int),
                ("rel_res_implicit", C.c_double), ("rel_res_explicit", C.c_double),
                ("prec_setup_ms", C.c_double), ("solve_ms", C.c_double), ("spmv_ms", C.c_double),
                ("spmv_calls", C.c_int), ("reorth", C.c_int), ("residual_restarts", C.c_int)]


class OrderGeometry(C.Structure):
    """isph_order_geometry: what the library's brick sort of the owned particles was made with (isph_mat_ordering_info)."""
    _fields_ = [("dim", C.c_int), ("lo", C.c_double * 3), ("inv_bin", C.c_double * 3), ("nbins", C.c_int * 3), ("ncell", C.c_int * 3),
                ("cells_per_brick", C.c_int * 3), ("nbrick", C.c_int * 3), ("shift", C.c_double * 3), ("period", C.c_double * 3)]


ORDERINGS = {"caller": 0, "bricks": 1}
# Row numbering of the contexts this binding creates when the caller does not say: None = the library's default
# (ISPH_ORDER_BRICKS: the assembly sorts the owned particles into bricks itself).  tests/conftest.py sets "caller" for the
# suites that compare internals (ILU factors, AMG aggregates) row by row with the oracle in the generator's numbering.
DEFAULT_ORDERING = None


class _Particles(C.Structure):
    _fields_ = [("dim", C.c_int), ("nlocal", C.c_int), ("nall", C.c_int), ("ntypes", C.c_int),
                ("kernel", C.c_int), ("x", C.c_void_p), ("type", C.c_void_p), ("kind", C.c_void_p),
                ("h", C.c_void_p), ("cutsq", C.c_void_p), ("neigh_ptr", C.c_void_p), ("neigh_idx", C.c_void_p),
                ("colmap", C.c_void_p), ("vfrac", C.c_void_p), ("Gc", C.c_void_p), ("Lc", C.c_void_p),
                ("morris_holmes", C.c_int), ("pnd", C.c_void_p), ("morris_safe_coeff", C.c_double),
                ("normal", C.c_void_p), ("solid_normal_diag", C.c_double), ("neigh_ptr64", C.c_void_p)]


_lib = None


def lib_path():
    return _build.HIP_LIB


def lib():
    """Loads libisph_hip.so; raises (never falls back) if it is not there."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError("libisph_hip.so is missing (%s): run __graft_entry__.build(); "
                               "there is no CPU fallback" % path)
        # When torch is in the process, load it first so both bind to ONE HIP/RCCL runtime
        # (torch ships its own libamdhip64/librccl; two runtimes in one process do not share the device).
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(path)
        L.isph_last_error.restype = C.c_char_p
        L.isph_prec_nnz.restype = C.c_longlong
        L.isph_prec_nnz.argtypes = [C.c_void_p]
        L.isph_ctx_create.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
        L.isph_ctx_create_dist.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_void_p]
        L.isph_ctx_create_hostcomm.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.isph_ctx_sync.argtypes = [C.c_void_p]
        L.isph_ctx_destroy.argtypes = [C.c_void_p]
        L.isph_pool_trim.argtypes = []
        L.isph_halo_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.isph_halo_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.isph_halo_destroy.argtypes = [C.c_void_p]
        L.isph_halo_destroy.restype = None
        L.isph_prec_create_overlap.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.isph_pool_set_cap.argtypes = [C.c_longlong]
        L.isph_set_exact_stream_threshold.argtypes = [C.c_longlong]
        L.isph_ingress_info.argtypes = [C.c_void_p, C.c_void_p]
        L.isph_pool_info.argtypes = [C.c_void_p, C.c_int]
        L.isph_pool_cached_bytes.argtypes = []
        L.isph_pool_cached_bytes.restype = C.c_longlong
        L.isph_ctx_set_profile.argtypes = [C.c_void_p, C.c_int]
        L.isph_ctx_hold_neighbours.argtypes = [C.c_void_p, C.c_int]
        L.isph_ctx_profile_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.isph_ctx_halo_profile_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.isph_ctx_comm_info.argtypes = [C.c_void_p, C.c_void_p]
        L.isph_device_identity.argtypes = [C.c_int, C.c_char_p]
        L.isph_ctx_set_ordering.argtypes = [C.c_void_p, C.c_int]
        L.isph_ctx_set_periodic_box.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.isph_mat_ordering_info.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.isph_mat_ordering.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.isph_mat_ordering_faces.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.isph_mat_create_csr.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_int, C.c_void_p]
        L.isph_mat_create_csr_bjacobi.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_int, C.c_void_p, C.c_void_p]
        L.isph_mat_create_csr_blocks.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.isph_mat_create_csr_coords.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.isph_mat_create_csr_coords_bjacobi.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.isph_mat_set_halo.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]
        L.isph_mat_info.argtypes = [C.c_void_p, C.c_void_p]
        L.isph_mat_export_csr.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.isph_mat_export_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]
        L.isph_mat_column_bits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.isph_mat_destroy.argtypes = [C.c_void_p]
        L.isph_spmv.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.isph_spmv_time.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.isph_prec_create.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int, C.c_void_p]
        L.isph_prec_create_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.isph_prec_create_blocks_fill.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.isph_prec_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.isph_prec_apply_multi.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.isph_prec_multi_path.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.isph_prec_export_ilu.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.isph_prec_destroy.argtypes = [C.c_void_p]
        L.isph_prec_info.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.isph_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                 C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.isph_assemble_poisson.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                            C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.isph_compute_volumes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.isph_compute_pnd.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.isph_compute_corrections.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        for fn in (L.isph_gradient, L.isph_divergence):
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_int,
                           C.c_void_p, C.c_int]
        L.isph_correct_velocity_pressure.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.isph_advance_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_int]
        L.isph_advance_end.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int]
        L.isph_assemble_block_helmholtz.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                    C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                    C.c_int]
        L.isph_solve_block.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_int]
        L.isph_prec_create_schwarz.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.isph_prec_schwarz_info.argtypes = [C.c_void_p, C.c_void_p]
        L.isph_prec_schwarz_paths.argtypes = [C.c_void_p, C.c_void_p]
        L.isph_prec_schwarz_export.argtypes = [C.c_void_p] * 7
        L.isph_prec_schwarz_timing.argtypes = [C.c_void_p, C.c_void_p]
        L.isph_amg_params_default.argtypes = [C.c_void_p]
        L.isph_prec_create_amg.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.isph_prec_amg_levels.argtypes = [C.c_void_p]
        L.isph_cheb_params_default.argtypes = [C.c_void_p]
        L.isph_prec_create_chebyshev.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.isph_prec_value_bits.argtypes = [C.c_void_p]
        L.isph_prec_eig_estimate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.isph_poly_params_default.argtypes = [C.c_void_p]
        L.isph_poly_params_default.restype = None
        L.isph_prec_create_gmres_poly.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.isph_prec_poly_info.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.isph_prec_type_kind.argtypes = [C.c_char_p]
        L.isph_prec_type_kind.restype = C.c_int
        L.isph_ilu_params_default.argtypes = [C.c_void_p]
        L.isph_ilu_params_default.restype = None
        L.isph_prec_create_ilu.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.isph_prec_value_bits.restype = C.c_int
        L.isph_prec_cycle_bits.argtypes = [C.c_void_p]
        L.isph_prec_cycle_bits.restype = C.c_int
        L.isph_prec_amg_info.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.isph_prec_amg_export.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.isph_prec_amg_aggregates.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.isph_prec_amg_path.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.isph_prec_amg_refreshes.argtypes = [C.c_void_p]
        L.isph_prec_amg_refreshes.restype = C.c_longlong
        L.isph_prec_amg_set_nullvec.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.isph_compute_shift.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_int]
        L.isph_apply_shift.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int]
        L.isph_shift_particles.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_double,
                                           C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_int]
        L.isph_assemble_helmholtz.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                              C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        L.isph_assemble_solute_transport.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double,
                                                     C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.isph_assemble_applied_potential.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                      C.c_void_p, C.c_void_p, C.c_int]
        L.isph_pb_params_default.argtypes = [C.c_void_p]
        L.isph_pb_params_default.restype = None
        L.isph_assemble_poisson_boltzmann.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                      C.c_void_p, C.c_int]
        L.isph_pb_residual.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.isph_pb_jacobian.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.isph_solve_poisson_boltzmann.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_int]
        L.isph_compute_normals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.isph_csf_params_default.argtypes = [C.c_void_p]
        L.isph_csf_params_default.restype = None
        L.isph_csf_phase_normal.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_int]
        L.isph_csf_force.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.isph_surface_tension_csf.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_int]
        L.isph_pairwise_force.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_int]
        L.isph_smooth_field.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
        L.isph_ek_params_default.argtypes = [C.c_void_p]
        L.isph_ek_params_default.restype = None
        L.isph_electrostatic_force.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_int]
        L.isph_random_stress_tensor.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_ulonglong, C.c_ulonglong, C.c_void_p,
                                                C.c_int]
        L.isph_random_stress_force.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_int]
        L.isph_force_from_random_stress.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_ulonglong,
                                                    C.c_ulonglong, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, C.c_int]
        L.isph_nlist_build.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
                                       C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.isph_nlist_info.argtypes = [C.c_void_p, C.c_void_p]
        L.isph_nlist_get.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.isph_nlist_destroy.argtypes = [C.c_void_p, C.c_void_p]
        L.isph_nlist_build_dist.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_int,
                                            C.POINTER(C.c_void_p)]
        L.isph_nlist_dist_info.argtypes = [C.c_void_p, C.c_void_p]
        L.isph_nlist_dist_get.argtypes = [C.c_void_p, C.c_void_p] + [C.c_void_p] * 6 + [C.c_int]
        L.isph_nlist_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.isph_nlist_forward_int.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.isph_migrate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                   C.POINTER(C.c_void_p)]
        L.isph_migrated_info.argtypes = [C.c_void_p, C.c_void_p]
        L.isph_migrated_get.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.isph_migrated_destroy.argtypes = [C.c_void_p, C.c_void_p]
        L.isph_ctx_hold_pattern.argtypes = [C.c_void_p, C.c_int]
        L.isph_mat_update_values.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.isph_mat_pattern_info.argtypes = [C.c_void_p, C.c_void_p]
        L.isph_prec_refactor.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.isph_recycle_create.argtypes = [C.c_void_p, C.c_void_p]
        L.isph_recycle_destroy.argtypes = [C.c_void_p]
        L.isph_recycle_destroy.restype = None
        L.isph_recycle_reset.argtypes = [C.c_void_p]
        L.isph_recycle_info.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.isph_recycle_export.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.isph_recycle_import.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.isph_solve_recycle.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                         C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.isph_dense_tall_gemm.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p,
                                           C.c_longlong, C.c_int, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int]
        L.isph_dense_block_gram.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p,
                                            C.c_longlong, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_int]
        L.isph_ghost_fill.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.isph_zero_mean_pressure.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                              C.c_void_p, C.c_int]
        L.isph_status.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
                                  C.c_int]
        L.isph_tgv_error.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_double, C.c_double, C.c_void_p, C.c_int]
        L.isph_ins_params_default.argtypes = [C.c_void_p]
        L.isph_ins_params_default.restype = None
        L.isph_ins_create.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.isph_ins_destroy.argtypes = [C.c_void_p]
        L.isph_ins_destroy.restype = None
        L.isph_ins_set_state.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int]
        L.isph_ins_set_list.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int]
        for fn in (L.isph_ins_rebuild, L.isph_ins_pre, L.isph_ins_advance):
            fn.argtypes = [C.c_void_p]
        L.isph_ins_sizes.argtypes = [C.c_void_p, C.c_void_p]
        L.isph_ins_get.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_int]
        L.isph_ins_view.argtypes = [C.c_void_p, C.c_void_p]
        L.isph_ins_force.argtypes = [C.c_void_p]
        L.isph_ins_force.restype = C.c_void_p
        L.isph_ins_add_force.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.isph_ins_solve.argtypes = [C.c_void_p, C.c_void_p]
        L.isph_ins_shift.argtypes = [C.c_void_p, C.c_void_p]
        L.isph_ins_diagnostics.argtypes = [C.c_void_p, C.c_double, C.c_void_p]
        L.isph_ins_run.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.isph_nlist_forward_multi.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.isph_zero_mean_pressure_dist.argtypes = L.isph_zero_mean_pressure.argtypes
        L.isph_status_dist.argtypes = L.isph_status.argtypes
        L.isph_tgv_error_dist.argtypes = L.isph_tgv_error.argtypes
        L.isph_ins_create_dist.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.isph_ins_set_state_dist.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.c_int]
        L.isph_ins_sizes_dist.argtypes = [C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


class IsphError(RuntimeError):
    pass


class OperandError(IsphError, ValueError):
    """an operand shorter than what the C ABI reads: refused by the binding before any library call"""


def _check(rc):
    if rc != 0:
        raise IsphError(lib().isph_last_error().decode() or "isph call failed")


def _is_torch(a):
    return type(a).__module__.startswith("torch")


def _ptr(a):
    if a is None:
        return None
    if _is_torch(a):
        assert a.is_contiguous()
        return C.c_void_p(a.data_ptr())
    return a.ctypes.data_as(C.c_void_p)


def _on_device(*arrs):
    flags = {bool(_is_torch(a) and a.is_cuda) for a in arrs if a is not None}
    if len(flags) != 1:
        raise ValueError("mix of host and device arrays")
    return int(flags.pop())


def _i32(a):
    if _is_torch(a):
        assert str(a.dtype) == "torch.int32", "int32 tensor expected, got %s" % a.dtype
        return a
    return np.ascontiguousarray(a, dtype=np.int32)


def _f64(a):
    if _is_torch(a):
        assert str(a.dtype) == "torch.float64", "float64 tensor expected, got %s" % a.dtype
        return a
    return np.ascontiguousarray(a, dtype=np.float64)


def device_identity(device=0):
    """isph_device_identity: the PCI bus id of HIP device `device` as this process sees it"""
    buf = C.create_string_buffer(64)
    _check(lib().isph_device_identity(int(device), buf))
    return buf.value.decode()


def pool_trim():
    """Return the device buffers the library keeps for the next set-up to the driver (isph_pool_trim)."""
    _check(lib().isph_pool_trim())


def ingress_info(ctx):
    """isph_ingress_info: milestones of the context's last host-side matrix ingress (ms), bytes that crossed the link."""
    a = (C.c_double * 8)()
    _check(lib().isph_ingress_info(ctx.h, a))
    return dict(staged_ms=a[0], queued_ms=a[1], copied_ms=a[2], device_done_ms=a[3], end_ms=a[4], waited_for_staging_ms=a[5],
                link_bytes=int(a[6]), threads=int(a[7]))


def pool_set_cap(nbytes):
    """Limit the library's cache of freed device blocks (isph_pool_set_cap; <= 0 restores the default of 80 % of the
    memory that was free at the first release).  torch's caching allocator does not see this cache: a process that
    lets torch allocate large tensors next to the library either caps it here or calls pool_trim() when
    torch.cuda.OutOfMemoryError is raised and retries."""
    _check(lib().isph_pool_set_cap(int(nbytes)))


def set_exact_stream_threshold(nbytes):
    """isph_set_exact_stream_threshold: ILU / Gauss-Seidel streams whose capacity-rule reservation exceeds nbytes are sized
    by a counting pass instead (default 4 GiB; 0 = always exact; < 0 = default)."""
    _check(lib().isph_set_exact_stream_threshold(int(nbytes)))


def pool_info(reset_peak=False):
    """isph_pool_info: dict(cached, live, peak_live, cap) in bytes."""
    a = (C.c_longlong * 4)()
    _check(lib().isph_pool_info(a, int(reset_peak)))
    return dict(cached=a[0], live=a[1], peak_live=a[2], cap=a[3])


def pool_cached_bytes():
    return int(lib().isph_pool_cached_bytes())


class HostTransport(C.Structure):
    """isph_host_transport: the two callbacks of a host-staged communicator (isph_ctx_create_hostcomm)."""
    _fields_ = [("user", C.c_void_p), ("exchange", C.c_void_p), ("allreduce", C.c_void_p)]


class Context:
    """isph_ctx: device + stream (+ RCCL communicator when nranks > 1, or the host-staged transport `transport`, a
    HostTransport whose callbacks outlive the context, for ranks that share a device)."""

    def __init__(self, device=0, stream=None, rank=0, nranks=1, uid=None, transport=None, ordering=None):
        """ordering: "bricks" (the library numbers the matrix rows itself, isph_ctx_set_ordering) | "caller" | None =
        DEFAULT_ORDERING, else the library's default (bricks)"""
        self.h = C.c_void_p()
        self.rank, self.nranks = rank, nranks
        if stream is None and "torch" in sys.modules:
            # default to the stream torch is issuing on, so zero-fills / temporaries of the caller and the
            # library's kernels are stream-ordered
            import torch
            if torch.cuda.is_available():
                stream = torch.cuda.current_stream(device).cuda_stream
        # handle 0 is the legacy null stream: the library then creates its own stream with hipStreamDefault,
        # i.e. one that is implicitly ordered against null-stream work (isph_capi.hip ctx_create_common)
        sp = C.c_void_p(stream) if stream else None
        if transport is not None:
            _check(lib().isph_ctx_create_hostcomm(device, sp, rank, nranks, C.byref(transport), C.byref(self.h)))
        elif nranks > 1 or uid is not None:
            _check(lib().isph_ctx_create_dist(device, sp, rank, nranks, uid, C.byref(self.h)))
        else:
            _check(lib().isph_ctx_create(device, sp, C.byref(self.h)))
        ordering = DEFAULT_ORDERING if ordering is None else ordering
        self.ordering = "bricks" if ordering is None else ordering
        if ordering is not None:
            self.set_ordering(ordering)

    def set_ordering(self, mode):
        """isph_ctx_set_ordering: "bricks" | "caller" for the matrices assembled from now on"""
        _check(lib().isph_ctx_set_ordering(self.h, ORDERINGS[mode]))
        self.ordering = mode

    def set_periodic_box(self, lo=None, hi=None, periodic=None):
        """isph_ctx_set_periodic_box: the caller's periodic box for the brick sort (None forgets it)"""
        if lo is None:
            _check(lib().isph_ctx_set_periodic_box(self.h, None, None, None))
            return
        a = (C.c_double * 3)(*[float(v) for v in (list(lo) + [0.0] * 3)[:3]])
        b = (C.c_double * 3)(*[float(v) for v in (list(hi) + [0.0] * 3)[:3]])
        p = (C.c_int * 3)(*[int(v) for v in (list(periodic) + [0] * 3)[:3]])
        _check(lib().isph_ctx_set_periodic_box(self.h, a, b, p))

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(UID_BYTES)
        _check(lib().isph_comm_unique_id(buf))
        return buf.raw

    def sync(self):
        _check(lib().isph_ctx_sync(self.h))

    def set_profile(self, on):
        _check(lib().isph_ctx_set_profile(self.h, int(on)))

    def hold_neighbours(self, on):
        """isph_ctx_hold_neighbours: while held, the operator calls share one layout of the (unchanged) neighbour list"""
        _check(lib().isph_ctx_hold_neighbours(self.h, int(on)))

    def hold_pattern(self, on):
        """isph_ctx_hold_pattern: while on, a matrix created from a CSR keeps the map of its entries (Matrix.update_values)
        and an ILU(k > 0) its fill levels (Precond.refactor)"""
        _check(lib().isph_ctx_hold_pattern(self.h, int(on)))

    PROFILE_CLASSES = ("spmv", "prec_apply", "multi_dot", "multi_axpy_dot", "multi_axpy_norm", "ilu_extract", "ilu_schedule",
                       "ilu_factor")

    def profile_read(self):
        """isph_ctx_profile_read: {class: (milliseconds, launches)} since the collection started; starts the next one"""
        ms, calls = (C.c_double * 8)(), (C.c_int * 8)()
        _check(lib().isph_ctx_profile_read(self.h, ms, calls))
        return {k: (ms[i], calls[i]) for i, k in enumerate(self.PROFILE_CLASSES)}

    def halo_profile_read(self):
        """isph_ctx_halo_profile_read: dict(products, exchange_ms, interior_ms, exposed_ms) summed since the collection started"""
        ms, calls = (C.c_double * 3)(), C.c_int()
        _check(lib().isph_ctx_halo_profile_read(self.h, ms, C.byref(calls)))
        return dict(products=calls.value, exchange_ms=ms[0], interior_ms=ms[1], exposed_ms=ms[2])

    def comm_info(self):
        """isph_ctx_comm_info: dict(transport "none" | "rccl" | "host", ranks, rank, device) -- for RCCL from the communicator"""
        a = (C.c_longlong * 4)()
        _check(lib().isph_ctx_comm_info(self.h, a))
        return dict(transport=("none", "rccl", "host")[int(a[0])], ranks=int(a[1]), rank=int(a[2]), device=int(a[3]))

    def close(self):
        if self.h:
            lib().isph_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HaloForward:
    """Stand-alone halo plan: forward comm of per-atom fields over the context's RCCL communicator
    (isph_halo_create / isph_halo_forward; LAMMPS' comm->forward_comm_pair for PairISPH, pair_isph.cpp:1924-2110)."""

    def __init__(self, ctx, nlocal, peers, send_ptr, send_idx, recv_ptr):
        self.ctx, self.nlocal = ctx, int(nlocal)
        peers, send_ptr, send_idx, recv_ptr = (np.ascontiguousarray(a, dtype=np.int32) for a in (peers, send_ptr, send_idx, recv_ptr))
        self.nrecv = int(recv_ptr[-1]) if len(recv_ptr) else 0
        self.h = C.c_void_p()
        _check(lib().isph_halo_create(ctx.h, self.nlocal, len(peers), _ptr(peers), _ptr(send_ptr), _ptr(send_idx), _ptr(recv_ptr),
                                      C.byref(self.h)))

    def forward(self, x, ncomp=1):
        """x: [nlocal] or [nlocal, ncomp] (numpy on the host or torch on the device) -> ghost values [nrecv(, ncomp)]
        in ghost-column order, on the same side as x."""
        dev = _on_device(x)
        x = _f64(x)
        assert x.shape[0] >= self.nlocal and (x.ndim == 1) == (ncomp == 1) and (x.ndim == 1 or x.shape[1] == ncomp)
        shape = (self.nrecv,) if ncomp == 1 else (self.nrecv, ncomp)
        if dev:
            import torch
            g = torch.empty(shape, dtype=torch.float64, device=x.device)
        else:
            g = np.empty(shape, dtype=np.float64)
        _check(lib().isph_halo_forward(self.ctx.h, self.h, _ptr(x), _ptr(g), int(ncomp), 1 if dev else 0))
        return g

    def close(self):
        if self.h:
            lib().isph_halo_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Matrix:
    """isph_mat: sliced-ELL device matrix (SolverLin::setMatrix ingress)."""

    def __init__(self, ctx, handle=None):
        self.ctx = ctx
        self.h = handle if handle is not None else C.c_void_p()

    @classmethod
    def from_csr(cls, ctx, rowptr, colidx, val, ncol=None):
        rowptr, colidx, val = _i32(rowptr), _i32(colidx), _f64(val)
        nrow = int(rowptr.shape[0]) - 1
        m = cls(ctx)
        _check(lib().isph_mat_create_csr(ctx.h, nrow, nrow if ncol is None else ncol, _ptr(rowptr), _ptr(colidx),
                                         _ptr(val), _on_device(rowptr, colidx, val), C.byref(m.h)))
        return m

    @classmethod
    def from_host_csr_with_coords(cls, ctx, rowptr, colidx, val, coords, dim=3, ncol=None, with_bjacobi=False):
        """isph_mat_create_csr_coords: host CSR in the caller's atom order + the coordinates of its rows ([nrow, >= dim]) ->
        a matrix in the library's own row numbering (the drop-in path with PrecondWrapper_Ifpack::setCoordinates).
        with_bjacobi: isph_mat_create_csr_coords_bjacobi, returns (Matrix, Precond) with the ILU(0) set-up of the library's
        bricks fused with the ingress"""
        rowptr, colidx, val = _i32(rowptr), _i32(colidx), _f64(val)
        nrow = int(rowptr.shape[0]) - 1
        xs = [np.ascontiguousarray(coords[:nrow, a], dtype=np.float64) for a in range(dim)]
        m = cls(ctx)
        if with_bjacobi:
            M = Precond.__new__(Precond)
            M.ctx, M.n, M.h = ctx, nrow, C.c_void_p()
            _check(lib().isph_mat_create_csr_coords_bjacobi(ctx.h, nrow, nrow if ncol is None else ncol, _ptr(rowptr), _ptr(colidx),
                                                            _ptr(val), int(dim), _ptr(xs[0]), _ptr(xs[1]),
                                                            _ptr(xs[2]) if dim == 3 else None, C.byref(m.h), C.byref(M.h)))
            return m, M
        _check(lib().isph_mat_create_csr_coords(ctx.h, nrow, nrow if ncol is None else ncol, _ptr(rowptr), _ptr(colidx), _ptr(val),
                                                int(dim), _ptr(xs[0]), _ptr(xs[1]), _ptr(xs[2]) if dim == 3 else None, C.byref(m.h)))
        return m

    @classmethod
    def from_host_csr_with_bjacobi(cls, ctx, rowptr, colidx, val, block_size=512, ncol=None, block_ptr=None):
        """isph_mat_create_csr_bjacobi: host CSR ingress fused with the block-Jacobi ILU(0) set-up (the drop-in path of
        SolverLin_Belos::solveProblem with PrecondWrapper_Ifpack).  block_ptr: the caller's subdomains
        (isph_mat_create_csr_blocks).  Returns (Matrix, Precond)."""
        rowptr, colidx, val = _i32(rowptr), _i32(colidx), _f64(val)
        if _is_torch(rowptr) or _is_torch(colidx) or _is_torch(val):
            raise IsphError("isph_mat_create_csr_bjacobi takes host arrays")
        nrow = int(rowptr.shape[0]) - 1
        m = cls(ctx)
        M = Precond.__new__(Precond)
        M.ctx, M.n, M.h = ctx, nrow, C.c_void_p()
        if block_ptr is not None:
            bp = np.ascontiguousarray(block_ptr, dtype=np.int32)
            _check(lib().isph_mat_create_csr_blocks(ctx.h, nrow, nrow if ncol is None else ncol, _ptr(rowptr), _ptr(colidx),
                                                    _ptr(val), len(bp) - 1, _ptr(bp), C.byref(m.h), C.byref(M.h)))
            return m, M
        _check(lib().isph_mat_create_csr_bjacobi(ctx.h, nrow, nrow if ncol is None else ncol, _ptr(rowptr), _ptr(colidx),
                                                 _ptr(val), block_size, C.byref(m.h), C.byref(M.h)))
        return m, M

    def set_halo(self, peers, send_ptr, send_idx, recv_ptr):
        peers, send_ptr, send_idx, recv_ptr = map(lambda a: np.ascontiguousarray(a, dtype=np.int32),
                                                  (peers, send_ptr, send_idx, recv_ptr))
        _check(lib().isph_mat_set_halo(self.ctx.h, self.h, len(peers), _ptr(peers), _ptr(send_ptr), _ptr(send_idx),
                                       _ptr(recv_ptr)))
        self._halo = True

    def info(self):
        a = (C.c_longlong * 6)()
        _check(lib().isph_mat_info(self.h, a))
        return dict(nrow=a[0], ncol=a[1], nnz=a[2], nslices=a[3], stored=a[4], sell_bytes=a[5])

    def ordering(self):
        """None for a matrix in the caller's row numbering; else dict(perm [nrow]: the caller's row held by internal row r,
        block_ptr: the library's subdomains over internal rows, geom: OrderGeometry, faces: the cell faces of the three axes)
        -- isph_mat_ordering(_info), isph_mat_ordering_faces."""
        a = (C.c_longlong * 3)()
        g = OrderGeometry()
        _check(lib().isph_mat_ordering_info(self.h, a, C.byref(g)))
        if not a[0]:
            return None
        perm = np.zeros(int(a[1]), dtype=np.int32)
        bp = np.zeros(int(a[2]) + 1, dtype=np.int32)
        _check(lib().isph_mat_ordering(self.ctx.h, self.h, _ptr(perm), _ptr(bp)))
        faces = []
        for ax in range(3):
            f = np.zeros(max(int(g.ncell[ax]) - 1, 0))
            if ax < g.dim and len(f):
                _check(lib().isph_mat_ordering_faces(self.h, ax, _ptr(f)))
            faces.append(f)
        return dict(perm=perm, block_ptr=bp, geom=g, faces=faces)

    def subdomains(self):
        """the library's subdomain table alone (no copy of the permutation); None for a matrix in the caller's numbering"""
        a = (C.c_longlong * 3)()
        _check(lib().isph_mat_ordering_info(self.h, a, None))
        if not a[0]:
            return None
        bp = np.zeros(int(a[2]) + 1, dtype=np.int32)
        _check(lib().isph_mat_ordering(self.ctx.h, self.h, None, _ptr(bp)))
        return bp

    def export_csr(self):
        i = self.info()
        rp = np.zeros(i["nrow"] + 1, dtype=np.int32)
        ci = np.zeros(i["nnz"], dtype=np.int32)
        v = np.zeros(i["nnz"])
        _check(lib().isph_mat_export_csr(self.ctx.h, self.h, _ptr(rp), _ptr(ci), _ptr(v)))
        return rp, ci, v

    def export_rows(self, row_begin, nrows, capacity=None):
        """isph_mat_export_rows: rows [row_begin, row_begin + nrows) as (rowptr int64 relative, colidx, val)."""
        cap = int(capacity if capacity is not None else nrows * 4096)
        rp = np.zeros(nrows + 1, dtype=np.int64)
        ci = np.zeros(cap, dtype=np.int32)
        v = np.zeros(cap)
        _check(lib().isph_mat_export_rows(self.ctx.h, self.h, int(row_begin), int(nrows), _ptr(rp), _ptr(ci), _ptr(v), cap))
        return rp, ci[:rp[-1]], v[:rp[-1]]

    def column_bits(self):
        """isph_mat_column_bits: 16 when the product reads the windowed 16-bit columns (built on first use), else 32"""
        b = C.c_int()
        _check(lib().isph_mat_column_bits(self.ctx.h, self.h, C.byref(b)))
        return b.value

    def update_values(self, val):
        """isph_mat_update_values: nnz new values (numpy on the host or a torch tensor on the device) in the entry order of
        the arrays the matrix was created from; needs the map of Context.hold_pattern(True)"""
        val = _f64(val)
        _need(val, self.info()["nnz"], "val [nnz]")
        _check(lib().isph_mat_update_values(self.ctx.h, self.h, _ptr(val), _on_device(val)))

    def pattern_info(self):
        """isph_mat_pattern_info: (1 when the matrix carries an entry map, bytes of the map, value updates taken)"""
        a = (C.c_longlong * 3)()
        _check(lib().isph_mat_pattern_info(self.h, a))
        return int(a[0]), int(a[1]), int(a[2])

    def sampled_product(self, x, nsamples=64, rows_per_sample=64, seed=0):
        """(A x) on `nsamples` runs of `rows_per_sample` consecutive rows, computed ON THE HOST from exported rows: an
        operator application that shares nothing with the SpMV kernels.  Returns (row indices, values)."""
        n = self.info()["nrow"]
        xh = x.detach().cpu().numpy() if _is_torch(x) else np.asarray(x)
        rng = np.random.default_rng(seed)
        starts = np.unique(np.minimum(rng.integers(0, max(n - rows_per_sample, 0) + 1, size=nsamples), max(n - rows_per_sample, 0)))
        rows, vals, mags = [], [], []
        for s0 in starts:
            m = min(rows_per_sample, n - int(s0))
            rp, ci, v = self.export_rows(int(s0), m)
            prod = v * xh[ci]
            vals.append(np.add.reduceat(prod, rp[:-1]) * (np.diff(rp) > 0) if len(prod) else np.zeros(m))
            mags.append(np.add.reduceat(np.abs(prod), rp[:-1]) * (np.diff(rp) > 0) if len(prod) else np.zeros(m))
            rows.append(np.arange(int(s0), int(s0) + m))
        self.last_sample_magnitude = np.concatenate(mags)     # sum_j |a_ij x_j| per sampled row: the scale of its round-off
        return np.concatenate(rows), np.concatenate(vals)

    def spmv(self, x, y=None):
        x = _f64(x)
        inf = self.info()
        # ghost columns without a halo plan: the caller supplies all ncol entries; otherwise the nrow owned ones
        _need(x, inf["ncol"] if (inf["ncol"] > inf["nrow"] and not getattr(self, "_halo", False)) else inf["nrow"], "x")
        _need(y, inf["nrow"], "y [nrow]")
        if y is None:
            n = self.info()["nrow"]
            if _is_torch(x):
                import torch
                y = torch.empty(n, dtype=torch.float64, device=x.device)
            else:
                y = np.zeros(n)
        _check(lib().isph_spmv(self.ctx.h, self.h, _ptr(x), _ptr(y), _on_device(x, y)))
        return y

    def spmv_time(self, x, y, reps=20, variant=0):
        ms = C.c_double()
        _check(lib().isph_spmv_time(self.ctx.h, self.h, _ptr(x), _ptr(y), reps, int(variant), C.byref(ms)))
        return ms.value

    def close(self):
        if self.h:
            lib().isph_mat_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Precond:
    """isph_prec == PrecondWrapper_Ifpack::create() result."""

    def __init__(self, ctx, A, kind="bjacobi-ilu0", block_size=512, block_ptr=None):
        """block_ptr: the caller's subdomains (isph_prec_create_blocks; kind must be "bjacobi-ilu0"): ascending row
        offsets from 0 to nrow, at most 1024 rows per subdomain.  block_size 0: the matrix' own subdomains (the bricks of
        the library's row numbering)"""
        self.ctx, self.n = ctx, A.info()["nrow"]
        self.h = C.c_void_p()
        self.A = A if kind.startswith(("chebyshev", "gmres-poly")) else None   # a polynomial applies the matrix: keep it alive
        if block_ptr is not None:
            f32 = kind.endswith("-f32")   # "bjacobi-ilu<k>-f32": the table form with value_bits = 32
            fill = kind[11:-4] if f32 else kind[11:]
            if not (kind.startswith("bjacobi-ilu") and fill.isdigit()):
                raise IsphError("unknown preconditioner type for a table of subdomains: %r (bjacobi-ilu<k>|bjacobi-ilu<k>-f32)" % kind)
            bp = np.ascontiguousarray(block_ptr, dtype=np.int32)
            if f32:
                prm = IluParams(level_of_fill=int(fill), nblocks=len(bp) - 1, block_ptr=bp.ctypes.data_as(C.POINTER(C.c_int)),
                                value_bits=32)
                _check(lib().isph_prec_create_ilu(ctx.h, A.h, C.byref(prm), C.byref(self.h)))
            else:
                _check(lib().isph_prec_create_blocks_fill(ctx.h, A.h, len(bp) - 1, _ptr(bp), int(fill), C.byref(self.h)))
        else:
            _check(lib().isph_prec_create(ctx.h, A.h, kind.encode(), block_size, C.byref(self.h)))

    def apply(self, r, z=None):
        r = _f64(r)
        _need(r, self.n, "r [n]"); _need(z, self.n, "z [n]")
        if z is None:
            if _is_torch(r):
                import torch
                z = torch.empty_like(r)
            else:
                z = np.zeros(self.n)
        _check(lib().isph_prec_apply(self.ctx.h, self.h, _ptr(r), _ptr(z), _on_device(r, z)))
        return z

    def apply_multi(self, R, Z=None, nvec=None, lda=None):
        """isph_prec_apply_multi: z_k = M^-1 r_k for several vectors, sharing the sweeps of M where the type has a one-sweep
        form (multi_path) -- the bits of one apply() per vector either way.  R (and Z) are column-major [lda x nvec] like
        the multivectors of solve(): a 2-D array / tensor [nvec, lda], or a flat one with nvec (and lda, default n) given.
        Rows n .. lda of Z are not written; a Z made here starts as zeros.  The element counts are checked before the call."""
        R = _f64(R)
        shape = tuple(R.shape)
        if len(shape) == 2:
            if nvec is None:
                nvec = shape[0]
            if lda is None:
                lda = shape[1]
        if nvec is None:
            raise OperandError("R is flat: nvec is needed")
        nvec, lda = int(nvec), int(self.n if lda is None else lda)
        if nvec < 1:
            raise OperandError("nvec = %d: at least one vector is needed" % nvec)
        if lda < self.n:
            raise OperandError("lda = %d is below the %d rows of the preconditioner" % (lda, self.n))
        if len(shape) == 2 and (shape[0] != nvec or shape[1] != lda):
            raise OperandError("R is %r, not [nvec = %d, lda = %d]" % (shape, nvec, lda))
        need = lda * (nvec - 1) + self.n
        _need(R, need, "R [lda x nvec]")
        if Z is None:
            if _is_torch(R):
                import torch
                Z = torch.zeros_like(R)
            else:
                Z = np.zeros_like(R)
        else:
            Z = _f64(Z)
        _need(Z, need, "Z [lda x nvec]")
        _check(lib().isph_prec_apply_multi(self.ctx.h, self.h, nvec, _ptr(R), _ptr(Z), lda, _on_device(R, Z)))
        return Z

    def multi_path(self, nvec):
        """isph_prec_multi_path: 1 when nvec vectors share the sweeps of this preconditioner (apply_multi, solve with
        nvec > 1, solve_block), 0 when they are applied one after the other"""
        return int(lib().isph_prec_multi_path(self.ctx.h, self.h, int(nvec)))

    def refactor(self, A):
        """isph_prec_refactor on the (updated) values of A.  "bjacobi-ilu<k>": the numeric factorisation again; pattern,
        schedule and layout are kept, the result is bit for bit a fresh create.  "chebyshev<d>" created under
        Context.hold_pattern(True): diagonal, rho or estimate and float plane again, bit for bit a fresh create.  "sa-amg" created under Context.hold_pattern(True), one rank: the
        hierarchy of the new values on the kept aggregates and patterns (a fresh create to round-off where it aggregates the
        same); a term without a slot in a kept pattern, another row count, a halo or a hierarchy created with the mode off
        are refused by name.  The preconditioner applies A from then on: it is kept alive here where the create call did."""
        _check(lib().isph_prec_refactor(self.ctx.h, self.h, A.h))
        if getattr(self, "A", None) is not None:
            self.A = A

    @property
    def value_bits(self):
        """isph_prec_value_bits: 32 or 64 = the width of the matrix values the Chebyshev sweeps read (the Chebyshev
        preconditioner, or an AMG with the Chebyshev smoother); 32 for a block ILU with single-precision stream values
        ("bjacobi-ilu<k>-f32"); 0 for every other preconditioner."""
        return int(lib().isph_prec_value_bits(self.h))

    @property
    def cycle_bits(self):
        """isph_prec_cycle_bits: 32 for an AMG built with AmgParams(cycle_bits=32) (the whole V cycle in single-precision
        storage: operators, level vectors and gathers float, arithmetic fp64; flexible GMRES only), 64 for everything else"""
        return int(lib().isph_prec_cycle_bits(self.h))

    def eig_estimate(self, level=0):
        """isph_prec_eig_estimate: lambda_used, rho = ||D^-1 A||_inf and the Arnoldi steps taken, for a Chebyshev
        preconditioner or level `level` of an AMG ({rho, rho, 0} with eig_type 0)"""
        a = (C.c_double * 3)()
        _check(lib().isph_prec_eig_estimate(self.ctx.h, self.h, int(level), a))
        return dict(lambda_used=float(a[0]), rho=float(a[1]), steps=int(a[2]))

    def _poly_info(self):
        roots = np.zeros(2 * POLY_MAX_DEGREE)
        hess = np.zeros((POLY_MAX_DEGREE + 1) * POLY_MAX_DEGREE)
        deg = C.c_int()
        _check(lib().isph_prec_poly_info(self.h, _ptr(roots), _ptr(hess), C.byref(deg)))
        return roots, hess, deg.value

    def roots(self):
        """isph_prec_poly_info: the roots of a GMRES polynomial ("gmres-poly<d>", PrecondGmresPoly) in application order, a
        complex array of the degree reached; any other kind fails by name"""
        roots, _, d = self._poly_info()
        return roots[0:2 * d:2] + 1j * roots[1:2 * d:2]

    def hessenberg(self):
        """isph_prec_poly_info: the Arnoldi matrix H, (degree + 1) x degree, of a GMRES polynomial"""
        _, hess, d = self._poly_info()
        return hess.reshape(POLY_MAX_DEGREE, POLY_MAX_DEGREE + 1).T[:d + 1, :d].copy()

    def info(self):
        a = (C.c_longlong * 4)()
        _check(lib().isph_prec_info(self.ctx.h, self.h, a))
        return dict(factor_nnz=a[0], stream_chunks=a[1], stream_capacity=a[2], nblocks=a[3])

    def export_ilu(self):
        nnz = lib().isph_prec_nnz(self.h)
        rp = np.zeros(self.n + 1, dtype=np.int32)
        ci = np.zeros(nnz, dtype=np.int32)
        v = np.zeros(nnz)
        _check(lib().isph_prec_export_ilu(self.ctx.h, self.h, _ptr(rp), _ptr(ci), _ptr(v)))
        return rp, ci, v

    def close(self):
        if self.h:
            lib().isph_prec_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IluParams(C.Structure):
    """Mirror of isph_ilu_params: level_of_fill 0..8; nblocks > 0 and block_ptr = the caller's table, else block_size rows
    per block (0: the matrix' own subdomains); value_bits 64 | 32 (the solves stream the factor values rounded to float)."""
    _fields_ = [("level_of_fill", C.c_int), ("block_size", C.c_int), ("nblocks", C.c_int), ("block_ptr", C.POINTER(C.c_int)),
                ("value_bits", C.c_int)]

    def __init__(self, **kw):
        super().__init__()
        lib().isph_ilu_params_default(C.byref(self))
        for k, v in kw.items():
            setattr(self, k, v)


class PrecondILU(Precond):
    """isph_prec_create_ilu: the block stream ("bjacobi-ilu<k>") from its parameter struct.  block_ptr: the caller's
    subdomains; otherwise block_size rows per block (0: the matrix' own subdomains).  value_bits = 32: the triangular
    solves read the strict-L / strict-U values rounded to float; the factor itself, the pivots and the vectors stay fp64."""

    def __init__(self, ctx, A, level_of_fill=0, block_size=0, block_ptr=None, value_bits=64):
        self.ctx, self.h, self.n, self.A = ctx, C.c_void_p(), A.info()["nrow"], None
        prm = IluParams(level_of_fill=int(level_of_fill), block_size=int(block_size), value_bits=int(value_bits))
        if block_ptr is not None:
            bp = np.ascontiguousarray(block_ptr, dtype=np.int32)
            prm.nblocks, prm.block_ptr = len(bp) - 1, bp.ctypes.data_as(C.POINTER(C.c_int))
        _check(lib().isph_prec_create_ilu(ctx.h, A.h, C.byref(prm), C.byref(self.h)))


class SchwarzParams(C.Structure):
    _fields_ = [("level_of_fill", C.c_int), ("overlap", C.c_int), ("combine", C.c_int), ("block_size", C.c_int),
                ("level_launches", C.c_int)]


class PrecondSchwarz(Precond):
    """isph_prec_create_schwarz: Ifpack_AdditiveSchwarz<ILU(k)> (precond_ifpack.h:28-75).  block_size 0 = one
    subdomain = the whole local matrix (the reference on one rank); combine "add" (reference) | "zero"."""

    def __init__(self, ctx, A, level_of_fill=1, overlap=1, combine="add", block_size=0, level_launches=False):
        self.ctx, self.h, self.n = ctx, C.c_void_p(), A.info()["nrow"]
        prm = SchwarzParams(int(level_of_fill), int(overlap), {"add": 0, "zero": 1}[combine], int(block_size),
                            int(bool(level_launches)))
        _check(lib().isph_prec_create_schwarz(ctx.h, A.h, C.byref(prm), C.byref(self.h)))

    def schwarz_info(self):
        a = (C.c_longlong * 7)()
        _check(lib().isph_prec_schwarz_info(self.h, a))
        return dict(nloc=a[0], nnz=a[1], nsub=a[2], levels_l=a[3], levels_u=a[4], maxrow=a[5], persistent=a[6])

    def paths(self):
        """which way the create call went (isph_prec_schwarz_paths)."""
        a = (C.c_longlong * 12)()
        _check(lib().isph_prec_schwarz_paths(self.h, a))
        return dict(rows_on_device=a[0], symbolic1_on_device=a[1], long_rows=a[2], factor_waves=a[3], hbits=a[4], nrun_l=a[5],
                    nrun_u=a[6], runs_near_l=a[7], runs_near_u=a[8], sub_maxrows=a[9], n4l=a[10], n4u=a[11])

    def create_timing(self):
        """ms of the create call by stage (isph_prec_schwarz_timing)."""
        a = (C.c_double * 6)()
        _check(lib().isph_prec_schwarz_timing(self.h, a))
        return dict(to_host=a[0], local_matrices=a[1], pattern=a[2], levels=a[3], upload=a[4], factor=a[5])

    def export(self):
        i = self.schwarz_info()
        rows = np.zeros(i["nloc"], dtype=np.int32)
        lp = np.zeros(i["nsub"] + 1, dtype=np.int32)
        rp = np.zeros(i["nloc"] + 1, dtype=np.int64)
        ci = np.zeros(i["nnz"], dtype=np.int32)
        v = np.zeros(i["nnz"])
        _check(lib().isph_prec_schwarz_export(self.ctx.h, self.h, _ptr(rows), _ptr(lp), _ptr(rp), _ptr(ci), _ptr(v)))
        return rows, lp, rp, ci, v


class PrecondOverlap(Precond):
    """isph_prec_create_overlap: ILU(k) of this rank's rows plus one layer of its neighbours' rows ("Overlap Level" 1 on
    more than one rank).  Aext: hip.Matrix of the extended subdomain (dist.extend_rows), plan: dist.HaloPlan."""

    def __init__(self, ctx, Aext, plan, level_of_fill=1, combine="add"):
        self.ctx, self.n = ctx, int(plan.nlocal)
        self.h = C.c_void_p()
        peers, sp, si, rp_ = (np.ascontiguousarray(a, dtype=np.int32) for a in (plan.peers, plan.send_ptr, plan.send_idx, plan.recv_ptr))
        _check(lib().isph_prec_create_overlap(ctx.h, Aext.h, self.n, int(level_of_fill), {"add": 0, "zero": 1}[combine],
                                              len(peers), _ptr(peers), _ptr(sp), _ptr(si), _ptr(rp_), C.byref(self.h)))


class ChebParams(C.Structure):
    """Mirror of isph_cheb_params: Ifpack's "chebyshev: degree", "chebyshev: ratio eigenvalue", "chebyshev: max eigenvalue",
    "chebyshev: min eigenvalue" (<= 0: from rho = ||D^-1 A||_inf); value_bits 64 | 32 (the polynomial of fl32(A));
    eig_type 0 | 1 (lambda_max <= 0: from rho | from eig_iters Arnoldi steps, clipped by rho)."""
    _fields_ = [("degree", C.c_int), ("ratio", C.c_double), ("lambda_max", C.c_double), ("lambda_min", C.c_double),
                ("value_bits", C.c_int), ("eig_type", C.c_int), ("eig_iters", C.c_int)]

    def __init__(self, **kw):
        super().__init__()
        lib().isph_cheb_params_default(C.byref(self))
        for k, v in kw.items():
            setattr(self, k, v)


class PrecondChebyshev(Precond):
    """isph_prec_create_chebyshev: Chebyshev polynomial in D^-1 A ("Precond Type" = "Chebyshev").  The matrix is applied,
    not copied: it is kept alive here.  value_bits = 32: the sweeps read the matrix values rounded to float (a plane the
    preconditioner owns); the result is the fp64 recurrence on fl32(A).  eig_type = 1: lambda from eig_iters Arnoldi steps
    on D^-1 A (clipped by rho) where lambda_max <= 0; .eig_estimate() reads it back."""

    def __init__(self, ctx, A, degree=1, ratio=30.0, lambda_max=0.0, lambda_min=0.0, value_bits=64, eig_type=0, eig_iters=10):
        self.ctx, self.h, self.n, self.A = ctx, C.c_void_p(), A.info()["nrow"], A
        prm = ChebParams(degree=int(degree), ratio=float(ratio), lambda_max=float(lambda_max), lambda_min=float(lambda_min),
                         value_bits=int(value_bits), eig_type=int(eig_type), eig_iters=int(eig_iters))
        _check(lib().isph_prec_create_chebyshev(ctx.h, A.h, C.byref(prm), C.byref(self.h)))


POLY_MAX_DEGREE = 25


class PolyParams(C.Structure):
    """Mirror of isph_poly_params: degree 1..25 of the GMRES polynomial (default 4)."""
    _fields_ = [("degree", C.c_int)]

    def __init__(self, **kw):
        super().__init__()
        lib().isph_poly_params_default(C.byref(self))
        for k, v in kw.items():
            setattr(self, k, v)


def prec_type_kind(kind):
    """isph_prec_type_kind: the kind a type string of Precond names (7 = "gmres-poly<d>"), -1 for one it refuses; no
    context and no device needed"""
    return int(lib().isph_prec_type_kind(str(kind).encode()))


class PrecondGmresPoly(Precond):
    """isph_prec_create_gmres_poly: Belos' GMRES polynomial of `degree` roots in D^-1 A as a fixed linear preconditioner.
    nullvec (host array or device tensor, the caller's row numbering): the null vector of a singular system; the set-up is
    projected with it.  The matrix is applied, not copied: it is kept alive here.  Precond(ctx, A, "gmres-poly<d>") is the
    same without a null vector."""

    def __init__(self, ctx, A, degree=4, nullvec=None):
        self.ctx, self.h, self.n, self.A = ctx, C.c_void_p(), A.info()["nrow"], A
        prm = PolyParams(degree=int(degree))
        nv = None if nullvec is None else _f64(nullvec)
        _need(nv, self.n, "nullvec [n]")
        _check(lib().isph_prec_create_gmres_poly(ctx.h, A.h, C.byref(prm), _ptr(nv), int(nv is not None and _is_torch(nv)),
                                                 C.byref(self.h)))


def solve_block(ctx, blocks, b, x, prec=None, params=None, lda=None):
    """isph_solve_block == SolverLin_Belos::solveBlockProblem.  blocks: dim x dim nested list of Matrix / None;
    b, x column-major [lda x dim] (numpy [dim, lda] arrays or flat); x is updated in place."""
    dim = len(blocks)
    arr = (C.c_void_p * (dim * dim))()
    n = None
    for i in range(dim):
        for j in range(dim):
            Bm = blocks[i][j]
            arr[i * dim + j] = Bm.h if Bm is not None else None
            if Bm is not None and n is None:
                n = Bm.info()["nrow"]
    prm = params or SolverParams()
    info = SolveInfo()
    _check(lib().isph_solve_block(ctx.h, dim, arr, prec.h if prec is not None else None, _ptr(b), _ptr(x),
                                  n if lda is None else lda, C.byref(prm), C.byref(info), _on_device(b, x)))
    return info


class PrecondAMG(Precond):
    """isph_prec_create_amg == PrecondWrapper_ML::create() (with setNullVector when nullvec is given).  eig_type / eig_iters
    (when given) replace the fields of params: 1 = every level's damping and Chebyshev interval from the Arnoldi estimate;
    .eig_estimate(level) reads the numbers back."""

    def __init__(self, ctx, A, nullvec=None, params=None, eig_type=None, eig_iters=None):
        self.ctx, self.n = ctx, A.info()["nrow"]
        self.h = C.c_void_p()
        prm = params or AmgParams()
        if eig_type is not None or eig_iters is not None:
            prm = AmgParams(**{k: getattr(prm, k) for k, _ in AmgParams._fields_})
            if eig_type is not None:
                prm.eig_type = int(eig_type)
            if eig_iters is not None:
                prm.eig_iters = int(eig_iters)
        nv = None if nullvec is None else _f64(nullvec)
        _check(lib().isph_prec_create_amg(ctx.h, A.h, C.byref(prm), _ptr(nv), int(nv is not None and _is_torch(nv)),
                                          C.byref(self.h)))

    @property
    def levels(self):
        return lib().isph_prec_amg_levels(self.h)

    def level_info(self, l):
        a = (C.c_longlong * 3)()
        _check(lib().isph_prec_amg_info(self.ctx.h, self.h, l, a))
        return dict(rows=int(a[0]), nnz=int(a[1]), nnz_p=int(a[2]))

    def export(self, l, what="A"):
        i = self.level_info(l)
        nnz = i["nnz"] if what == "A" else i["nnz_p"]
        rp = np.zeros(i["rows"] + 1, dtype=np.int32)
        ci = np.zeros(nnz, dtype=np.int32)
        v = np.zeros(nnz)
        _check(lib().isph_prec_amg_export(self.ctx.h, self.h, l, 0 if what == "A" else 1, _ptr(rp), _ptr(ci), _ptr(v)))
        return rp, ci, v

    def aggregates(self, l):
        a = np.zeros(self.level_info(l)["rows"], dtype=np.int32)
        _check(lib().isph_prec_amg_aggregates(self.ctx.h, self.h, l, _ptr(a)))
        return a

    def set_nullvec(self, nullvec):
        """isph_prec_amg_set_nullvec: new values for the null vector given at create, read by the next refactor()"""
        nv = _f64(nullvec)
        _need(nv, self.n, "nullvec [n]")
        _check(lib().isph_prec_amg_set_nullvec(self.ctx.h, self.h, _ptr(nv), int(_is_torch(nv))))

    @property
    def refreshes(self):
        """isph_prec_amg_refreshes: the refactor() calls this hierarchy has gone through"""
        return int(lib().isph_prec_amg_refreshes(self.h))

    PATH_KEYS = ("mis_rounds", "mis_list_rounds", "prolong", "ap", "galerkin", "smoother", "coarse", "prep")

    def path(self, l):
        """isph_prec_amg_path: which branch of every ladder the set-up took on level l (see include/isph_hip.h)"""
        a = (C.c_longlong * 8)()
        _check(lib().isph_prec_amg_path(self.ctx.h, self.h, l, a))
        return dict(zip(self.PATH_KEYS, (int(x) for x in a)))


class RecycleSpace:
    """isph_recycle: the recycle space of "Recycling GMRES" (solver_type 2) carried from one solve to the next --
    solve(..., recycle=space).  One object per sequence of systems; not a reference feature (include/isph_hip.h)."""
    REASONS = {0: "none", 1: "number of rows changed", 2: "orthonormalisation guard", 3: "more vectors than k + 1"}

    def __init__(self, ctx):
        self.ctx = ctx
        self.h = C.c_void_p()
        _check(lib().isph_recycle_create(ctx.h, C.byref(self.h)))

    def info(self):
        out = (C.c_longlong * 8)()
        _check(lib().isph_recycle_info(self.ctx.h, self.h, out))
        keys = ("n", "vectors", "started", "discarded", "last_reason", "applications", "steps", "bytes")
        return dict(zip(keys, (int(v) for v in out)))

    def export(self):
        """U [n x kk] in the caller's row numbering (numpy, Fortran order)"""
        i = self.info()
        U = np.zeros((i["n"], i["vectors"]), dtype=np.float64, order="F")
        if U.size:
            _check(lib().isph_recycle_export(self.ctx.h, self.h, _ptr(U)))
        return U

    def import_(self, U):
        """isph_recycle_import (diagnostic): U [n x kk] in the caller's row numbering replaces the space"""
        U = np.asfortranarray(U, dtype=np.float64)
        _check(lib().isph_recycle_import(self.ctx.h, self.h, int(U.shape[0]), int(U.shape[1]), _ptr(U)))

    def reset(self):
        _check(lib().isph_recycle_reset(self.h))

    def close(self):
        if self.h:
            lib().isph_recycle_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def dense_tall_gemm(ctx, n, A, lda, B, ldb, coef, out, ldo, mode=0):
    """isph_dense_tall_gemm (diagnostic): A [pa vectors], B [pb vectors or None], coef [(pa + pb) x q]; mode 0 set,
    1 accumulate into out, 2 in place (A <- A coef, coef upper triangular), 3 set by one launch per block and column"""
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    p, q = coef.shape
    pa = 0 if A is None else _count_vectors(A, n, lda)
    pb = 0 if B is None else _count_vectors(B, n, ldb)
    if pa + pb != p:
        raise OperandError("coef has %d rows for %d vectors" % (p, pa + pb))
    if mode != 2:
        _need(out, ldo * (q - 1) + n, "out [ldo x q]")
    _check(lib().isph_dense_tall_gemm(ctx.h, n, pa, _ptr(A), lda, pb, _ptr(B), ldb, q, _ptr(coef), _ptr(out), ldo, mode,
                                      _on_device(A, B, out)))
    return A if mode == 2 else out


def dense_block_gram(ctx, n, XA, lda, XB, ldb, Y, ldy, per_column=False):
    """isph_dense_block_gram (diagnostic): G [(pa + pb) x q] = [XA | XB]^T Y over n rows; per_column: by one multi-dot
    launch per block and column of Y"""
    pa = 0 if XA is None else _count_vectors(XA, n, lda)
    pb = 0 if XB is None else _count_vectors(XB, n, ldb)
    q = _count_vectors(Y, n, ldy)
    G = np.zeros((pa + pb, q), dtype=np.float64)
    _check(lib().isph_dense_block_gram(ctx.h, n, pa, _ptr(XA), lda, pb, _ptr(XB), ldb, q, _ptr(Y), ldy, _ptr(G),
                                       int(per_column), _on_device(XA, XB, Y)))
    return G


def _count_vectors(a, n, ld):
    """vectors of a vector-major block given as a flat array of ld (nv - 1) + n elements (or [nv, ld])"""
    have = int(a.numel()) if _is_torch(a) else int(np.asarray(a).size)
    if ld < max(n, 1):
        raise OperandError("leading dimension %d shorter than the vectors (%d)" % (ld, n))
    nv = (have - n) // ld + 1 if have >= n else 0
    if nv < 1:
        raise OperandError("block shorter than one vector")
    return nv


def solve(ctx, A, b, x, prec=None, singular=False, null_mask=None, params=None, nvec=1, lda=None, recycle=None):
    """isph_solve == SolverLin_Belos::solveProblem.  b and x are updated in
    place (b by its projection when singular); returns SolveInfo.  recycle: a RecycleSpace (solver_type 2 only) that
    carries the recycle space to the next solve -- isph_solve_recycle."""
    prm = params or SolverParams()
    info = SolveInfo()
    n = A.info()["nrow"]
    mask = None if null_mask is None else np.ascontiguousarray(null_mask, dtype=np.int32)
    ld = n if lda is None else lda
    _need(b, ld * (nvec - 1) + n, "b [lda x nvec]"); _need(x, ld * (nvec - 1) + n, "x [lda x nvec]"); _need(mask, n, "null_mask [n]")
    if recycle is not None:
        _check(lib().isph_solve_recycle(ctx.h, A.h, prec.h if prec is not None else None, _ptr(b), _ptr(x), nvec,
                                        n if lda is None else lda, int(singular), _ptr(mask), C.byref(prm), C.byref(info),
                                        _on_device(b, x), recycle.h))
        return info
    _check(lib().isph_solve(ctx.h, A.h, prec.h if prec is not None else None, _ptr(b), _ptr(x), nvec,
                            n if lda is None else lda, int(singular), _ptr(mask), C.byref(prm), C.byref(info),
                            _on_device(b, x)))
    return info


def _need(a, count, what):
    """operand of a C-ABI call: at least `count` elements (None passes)"""
    if a is None:
        return
    have = int(a.numel()) if _is_torch(a) else int(np.asarray(a).size)
    if have < count:
        raise OperandError("%s: %d elements given, %d needed" % (what, have, count))


def particles_view(parts, colmap, kernel="wendland", kinds=None, vfrac=None, Gc=None, Lc=None, keep=None,
                   pnd=None, morris_safe_coeff=0.43301, normal=None, solid_normal_diag=1.0):
    """Builds the isph_particles struct over host (numpy) or device (torch)
    arrays.  `keep` collects references so the buffers outlive the call."""
    keep = keep if keep is not None else []
    if kinds is not None:
        ntypes = len(kinds)
    elif int(parts["nall"]) == 0:                                  # a rank without particles (LAMMPS allows empty subdomains)
        ntypes = 1
    else:
        ntypes = int(np.max(parts["type"])) if not _is_torch(parts["type"]) else int(parts["type"].max().item())
    kind = np.ascontiguousarray([0] + list(kinds if kinds is not None else [99] * ntypes), dtype=np.int32)
    h = np.full((ntypes + 1, ntypes + 1), float(parts["h"]))
    cutsq = np.full((ntypes + 1, ntypes + 1), float(parts["cut"]) ** 2)
    x, typ = _f64(parts["x"]), _i32(parts["type"])
    nidx, cm = _i32(parts["neigh_idx"]), _i32(colmap)
    nptr_raw = parts["neigh_ptr"]
    wide = str(nptr_raw.dtype) in ("int64", "torch.int64")        # 64-bit list offsets -> isph_particles::neigh_ptr64
    nptr = (nptr_raw if _is_torch(nptr_raw) else np.ascontiguousarray(nptr_raw)) if wide else _i32(nptr_raw)
    pnd = None if pnd is None else _f64(pnd)
    normal = None if normal is None else _f64(normal)
    keep += [kind, h, cutsq, x, typ, nptr, nidx, cm, vfrac, Gc, Lc, pnd, normal]
    nl, na, dm = int(parts["nlocal"]), int(parts["nall"]), int(parts["dim"])
    # the C ABI takes bare pointers: a short array would be read past its end
    _need(x, 3 * na, "x [nall][3]"); _need(typ, na, "type [nall]"); _need(cm, na, "colmap [nall]")
    _need(nptr, nl + 1, "neigh_ptr [nlocal+1]"); _need(vfrac, na, "vfrac [nall]"); _need(pnd, na, "pnd [nall]")
    _need(Gc, nl * dm * dm, "Gc [nlocal][dim*dim]"); _need(Lc, nl * dm * (dm + 1) // 2, "Lc [nlocal][dimL]")
    _need(normal, 3 * na, "normal [nall][3]")
    pv = _Particles(int(parts["dim"]), int(parts["nlocal"]), int(parts["nall"]), ntypes, KERNELS[kernel],
                    _ptr(x), _ptr(typ), _ptr(kind), _ptr(h), _ptr(cutsq), None if wide else _ptr(nptr), _ptr(nidx), _ptr(cm),
                    _ptr(vfrac), _ptr(Gc), _ptr(Lc), int(pnd is not None), _ptr(pnd), float(morris_safe_coeff),
                    _ptr(normal), float(solid_normal_diag), _ptr(nptr) if wide else None)
    return pv, _on_device(x, typ, nptr, nidx, cm, vfrac, Gc, Lc, pnd, normal), keep


def assemble_poisson(ctx, parts, colmap, dt, rho, vstar, antisym=True, singular=NULLSPACE, rank0=True,
                     ncol=None, vfrac=None, kernel="wendland", b_out=None, kinds=None, pnd=None, Gc=None, Lc=None,
                     morris_safe_coeff=0.43301, normal=None, solid_normal_diag=1.0):
    """isph_assemble_poisson == PairISPH_Corrected::computePoisson."""
    keep = []
    pv, dev, keep = particles_view(parts, colmap, kernel=kernel, vfrac=vfrac, keep=keep, kinds=kinds, pnd=pnd, Gc=Gc,
                                   Lc=Lc, morris_safe_coeff=morris_safe_coeff, normal=normal,
                                   solid_normal_diag=solid_normal_diag)
    rho, vstar = _f64(rho), _f64(vstar)
    nlocal = int(parts["nlocal"])
    _need(rho, int(parts["nall"]), "rho [nall]"); _need(vstar, 3 * int(parts["nall"]), "vstar [nall][3]")
    if b_out is None:
        if dev:
            import torch
            b_out = torch.zeros(nlocal, dtype=torch.float64, device=rho.device)
        else:
            b_out = np.zeros(nlocal)
    A = Matrix(ctx)
    _check(lib().isph_assemble_poisson(ctx.h, C.byref(pv), int(antisym), float(dt), _ptr(rho), _ptr(vstar),
                                       singular, int(rank0), nlocal if ncol is None else ncol, C.byref(A.h),
                                       _ptr(b_out), dev))
    return A, b_out


def assemble_helmholtz(ctx, parts, colmap, dt, theta, nu, rho, pres, force, g, vel, antisym=True, incremental=True,
                       ncol=None, vfrac=None, Gc=None, Lc=None, kernel="wendland", kinds=None, pnd=None,
                       morris_safe_coeff=0.43301, rhs_only=False):
    """isph_assemble_helmholtz == PairISPH_Corrected::computeHelmholtz.  Returns (Matrix, b) with b
    column-major [nlocal x dim] flattened (component k at b[k*nlocal:(k+1)*nlocal])."""
    keep = []
    pv, dev, keep = particles_view(parts, colmap, kernel=kernel, vfrac=vfrac, Gc=Gc, Lc=Lc, keep=keep, kinds=kinds,
                                   pnd=pnd, morris_safe_coeff=morris_safe_coeff)
    nu, rho, pres, force, vel = map(_f64, (nu, rho, pres, force, vel))
    gv = np.ascontiguousarray(g, dtype=np.float64)
    nlocal, dim = int(parts["nlocal"]), int(parts["dim"])
    na = int(parts["nall"])
    for a_, c_, w_ in ((nu, na, "nu [nall]"), (rho, na, "rho [nall]"), (pres, na, "pres [nall]"), (force, 3 * na, "force [nall][3]"),
                       (vel, 3 * na, "v [nall][3]")):
        _need(a_, c_, w_)
    if dev:
        import torch
        b_out = torch.zeros(nlocal * dim, dtype=torch.float64, device=rho.device)
    else:
        b_out = np.zeros(nlocal * dim)
    A = None if rhs_only else Matrix(ctx)
    _check(lib().isph_assemble_helmholtz(ctx.h, C.byref(pv), int(antisym), float(dt), float(theta), _ptr(nu), _ptr(rho),
                                         _ptr(pres), _ptr(force), _ptr(gv), int(incremental), _ptr(vel),
                                         nlocal if ncol is None else ncol, None if rhs_only else C.byref(A.h),
                                         _ptr(b_out), nlocal, dev))
    return A, b_out


def assemble_solute_transport(ctx, parts, colmap, dt, theta, dcoeff, conc, antisym=True, ncol=None, vfrac=None, Gc=None,
                              Lc=None, kernel="wendland", kinds=None):
    """isph_assemble_solute_transport == PairISPH_Corrected::computeSoluteTransportSpecies.  Returns (Matrix, b[nlocal])."""
    keep = []
    pv, dev, keep = particles_view(parts, colmap, kernel=kernel, vfrac=vfrac, Gc=Gc, Lc=Lc, keep=keep, kinds=kinds)
    conc = _f64(conc)
    nlocal = int(parts["nlocal"])
    _need(conc, int(parts["nall"]), "conc [nall]")
    if dev:
        import torch
        b_out = torch.zeros(nlocal, dtype=torch.float64, device=conc.device)
    else:
        b_out = np.zeros(nlocal)
    A = Matrix(ctx)
    _check(lib().isph_assemble_solute_transport(ctx.h, C.byref(pv), int(antisym), float(dt), float(theta), float(dcoeff),
                                                _ptr(conc), nlocal if ncol is None else ncol, C.byref(A.h), _ptr(b_out), dev))
    return A, b_out


def assemble_applied_potential(ctx, parts, colmap, sigma, phi, antisym=True, ncol=None, vfrac=None, Gc=None, Lc=None,
                               kernel="wendland", kinds=None):
    """isph_assemble_applied_potential == PairISPH_Corrected::computeAppliedElectricPotential.  Returns (Matrix, b[nlocal])."""
    keep = []
    pv, dev, keep = particles_view(parts, colmap, kernel=kernel, vfrac=vfrac, Gc=Gc, Lc=Lc, keep=keep, kinds=kinds)
    phi = _f64(phi)
    sg = None if sigma is None else _f64(sigma)
    nlocal = int(parts["nlocal"])
    _need(phi, int(parts["nall"]), "phi [nall]"); _need(sg, int(parts["nall"]), "sigma [nall]")
    if dev:
        import torch
        b_out = torch.zeros(nlocal, dtype=torch.float64, device=phi.device)
    else:
        b_out = np.zeros(nlocal)
    A = Matrix(ctx)
    _check(lib().isph_assemble_applied_potential(ctx.h, C.byref(pv), int(antisym), _ptr(sg), _ptr(phi),
                                                 nlocal if ncol is None else ncol, C.byref(A.h), _ptr(b_out), dev))
    return A, b_out


def assemble_poisson_boltzmann(ctx, parts, colmap, eps=None, psi0=None, antisym=True, ncol=None, vfrac=None, Gc=None,
                               Lc=None, kernel="wendland", kinds=None, pnd=None, morris_safe_coeff=0.43301):
    """isph_assemble_poisson_boltzmann == the Laplacian part of FunctorOuterPoissonBoltzmannJacobian (the reference's
    A.is_filled pass).  eps, psi0: [nall] or None (1 / 0).  pnd given: the MorrisHolmes mirror.  Returns the Jacobian
    Matrix, which pb_residual / pb_jacobian / solve_poisson_boltzmann take."""
    keep = []
    pv, dev, keep = particles_view(parts, colmap, kernel=kernel, vfrac=vfrac, Gc=Gc, Lc=Lc, keep=keep, kinds=kinds,
                                   pnd=pnd, morris_safe_coeff=morris_safe_coeff)
    eps = None if eps is None else _f64(eps)
    psi0 = None if psi0 is None else _f64(psi0)
    nlocal, na = int(parts["nlocal"]), int(parts["nall"])
    _need(eps, na, "eps [nall]"); _need(psi0, na, "psi0 [nall]")
    J = Matrix(ctx)
    _check(lib().isph_assemble_poisson_boltzmann(ctx.h, C.byref(pv), int(antisym), _ptr(eps), _ptr(psi0),
                                                 nlocal if ncol is None else ncol, C.byref(J.h), dev))
    return J


def pb_residual(ctx, J, psi, f=None, params=None):
    """isph_pb_residual == computeF: F [nlocal] at psi [nlocal] (f: the Extra F [nlocal] or None)"""
    prm = params or PBParams()
    n = J.info()["nrow"]
    psi = _f64(psi)
    f = None if f is None else _f64(f)
    _need(psi, n, "psi [nlocal]"); _need(f, n, "f [nlocal]")
    dev = _on_device(psi, f)
    if dev:
        import torch
        F = torch.empty(n, dtype=torch.float64, device=psi.device)
    else:
        F = np.zeros(n)
    _check(lib().isph_pb_residual(ctx.h, J.h, C.byref(prm), _ptr(psi), _ptr(f), _ptr(F), dev))
    return F


def pb_jacobian(ctx, J, psi, params=None):
    """isph_pb_jacobian == computeJacobian: J's diagonal at psi [nlocal], in place"""
    prm = params or PBParams()
    psi = _f64(psi)
    _need(psi, J.info()["nrow"], "psi [nlocal]")
    _check(lib().isph_pb_jacobian(ctx.h, J.h, C.byref(prm), _ptr(psi), _on_device(psi)))


def solve_poisson_boltzmann(ctx, J, psi, f=None, params=None):
    """isph_solve_poisson_boltzmann == solveProblem: Newton from psi [nlocal] (updated in place: a contiguous float64
    numpy array or CUDA tensor); returns PBInfo"""
    prm = params or PBParams()
    info = PBInfo()
    n = J.info()["nrow"]
    f = None if f is None else _f64(f)
    _need(psi, n, "psi [nlocal]"); _need(f, n, "f [nlocal]")
    if _f64(psi) is not psi:
        raise ValueError("psi is updated in place: pass a contiguous float64 array")
    _check(lib().isph_solve_poisson_boltzmann(ctx.h, J.h, C.byref(prm), _ptr(f), _ptr(psi), C.byref(info),
                                              _on_device(psi, f)))
    return info


def assemble_block_helmholtz(ctx, parts, colmap, dt, theta, beta, nu, rho, pres, force, g, vel, normal=None, antisym=True,
                             incremental=True, ncol=None, vfrac=None, Gc=None, Lc=None, kernel="wendland", kinds=None,
                             pnd=None, morris_safe_coeff=0.43301):
    """isph_assemble_block_helmholtz == PairISPH_Corrected::computeBlockHelmholtz.  Returns (blocks, b): blocks is a
    dim x dim nested list of Matrix / None, b column-major [nlocal x dim] flattened."""
    keep = []
    pv, dev, keep = particles_view(parts, colmap, kernel=kernel, vfrac=vfrac, Gc=Gc, Lc=Lc, keep=keep, kinds=kinds,
                                   pnd=pnd, morris_safe_coeff=morris_safe_coeff)
    nu, rho, pres, force, vel = map(_f64, (nu, rho, pres, force, vel))
    nrm = None if normal is None else _f64(normal)
    na = int(parts["nall"])
    for a_, c_, w_ in ((nu, na, "nu [nall]"), (rho, na, "rho [nall]"), (pres, na, "pres [nall]"), (force, 3 * na, "force [nall][3]"),
                       (vel, 3 * na, "v [nall][3]"), (nrm, 3 * na, "normal [nall][3]")):
        _need(a_, c_, w_)
    gv = np.ascontiguousarray(g, dtype=np.float64)
    nlocal, dim = int(parts["nlocal"]), int(parts["dim"])
    if dev:
        import torch
        b_out = torch.zeros(nlocal * dim, dtype=torch.float64, device=rho.device)
    else:
        b_out = np.zeros(nlocal * dim)
    hs = (C.c_void_p * (dim * dim))()
    _check(lib().isph_assemble_block_helmholtz(ctx.h, C.byref(pv), int(antisym), float(dt), float(theta), float(beta),
                                               _ptr(nu), _ptr(rho), _ptr(pres), _ptr(force), _ptr(gv), int(incremental),
                                               _ptr(vel), _ptr(nrm), nlocal if ncol is None else ncol, hs, _ptr(b_out),
                                               nlocal, dev))
    blocks = [[None] * dim for _ in range(dim)]
    for i in range(dim):
        for j in range(dim):
            if hs[i * dim + j]:
                Bm = Matrix(ctx)
                Bm.h = C.c_void_p(hs[i * dim + j])
                blocks[i][j] = Bm
    return blocks, b_out


def compute_volumes(ctx, parts, colmap, kernel="wendland"):
    keep = []
    pv, dev, keep = particles_view(parts, colmap, kernel=kernel, keep=keep)
    nlocal = int(parts["nlocal"])
    if dev:
        import torch
        out = torch.zeros(nlocal, dtype=torch.float64, device=parts["x"].device)
    else:
        out = np.zeros(nlocal)
    _check(lib().isph_compute_volumes(ctx.h, C.byref(pv), _ptr(out), dev))
    return out


def compute_pnd(ctx, parts, colmap, kernel="wendland", kinds=None):
    """isph_compute_pnd: particle number density of the MorrisHolmes mirror (functor_normal.h:57-133); [nlocal]."""
    keep = []
    pv, dev, keep = particles_view(parts, colmap, kernel=kernel, keep=keep, kinds=kinds)
    nlocal = int(parts["nlocal"])
    if dev:
        import torch
        out = torch.zeros(nlocal, dtype=torch.float64, device=parts["x"].device)
    else:
        out = np.zeros(nlocal)
    _check(lib().isph_compute_pnd(ctx.h, C.byref(pv), _ptr(out), dev))
    return out


def compute_corrections(ctx, parts, colmap, vfrac, kernel="wendland"):
    """isph_compute_corrections == computeGradientCorrection + computeLaplacianCorrection.
    Returns (Gc [nlocal, dim*dim], Lc [nlocal, dimL])."""
    keep = []
    pv, dev, keep = particles_view(parts, colmap, kernel=kernel, vfrac=vfrac, keep=keep)
    nlocal, dim = int(parts["nlocal"]), int(parts["dim"])
    dL = dim * (dim + 1) // 2
    if dev:
        import torch
        G = torch.zeros((nlocal, dim * dim), dtype=torch.float64, device=parts["x"].device)
        Lc = torch.zeros((nlocal, dL), dtype=torch.float64, device=parts["x"].device)
    else:
        G, Lc = np.zeros((nlocal, dim * dim)), np.zeros((nlocal, dL))
    _check(lib().isph_compute_corrections(ctx.h, C.byref(pv), _ptr(G), _ptr(Lc), dev))
    return G, Lc


def _out_like(dev, ref, shape):
    """output buffer on the side the inputs live on (device tensors in -> device tensor out)"""
    if dev:
        import torch
        return torch.zeros(shape, dtype=torch.float64, device=ref.device)
    return np.zeros(shape)


def _same_side(dev, *arrays):
    """every operand of a call must live on the side the particle arrays live on"""
    for a in arrays:
        if a is not None and bool(_is_torch(a)) != bool(dev):
            raise ValueError("mixing host and device operands in one call")


def gradient(ctx, parts, colmap, f, vfrac, antisym=True, alpha=1.0, filt=None, Gc=None, kernel="wendland", kinds=None):
    """isph_gradient: scalar field f [nall] -> [nlocal, 3]."""
    keep = []
    pv, dev, keep = particles_view(parts, colmap, kernel=kernel, vfrac=vfrac, Gc=Gc, keep=keep, kinds=kinds)
    f = _f64(f)
    _same_side(dev, f)
    _need(f, int(parts["nall"]), "f [nall]")
    out = _out_like(dev, f, (int(parts["nlocal"]), 3))
    fi, fj = filt if filt is not None else (127, 127)
    _check(lib().isph_gradient(ctx.h, C.byref(pv), int(antisym), _ptr(f), float(alpha), int(filt is not None), fi, fj,
                               _ptr(out), dev))
    return out


def divergence(ctx, parts, colmap, f, vfrac, antisym=True, alpha=1.0, filt=None, Gc=None, kernel="wendland", kinds=None):
    """isph_divergence: vector field f [nall, 3] -> [nlocal]."""
    keep = []
    pv, dev, keep = particles_view(parts, colmap, kernel=kernel, vfrac=vfrac, Gc=Gc, keep=keep, kinds=kinds)
    f = _f64(f)
    _same_side(dev, f)
    _need(f, 3 * int(parts["nall"]), "f [nall][3]")
    out = _out_like(dev, f, (int(parts["nlocal"]),))
    fi, fj = filt if filt is not None else (127, 127)
    _check(lib().isph_divergence(ctx.h, C.byref(pv), int(antisym), _ptr(f), float(alpha), int(filt is not None), fi, fj,
                                 _ptr(out), dev))
    return out


def correct_velocity_pressure(ctx, parts, colmap, dt, rho, dp, vstar, p, vfrac, antisym=True, incremental=True, Gc=None,
                              kernel="wendland"):
    """in-place on vstar [nall,3] and p [nall] (numpy arrays or device tensors, like the particle arrays)."""
    keep = []
    pv, dev, keep = particles_view(parts, colmap, kernel=kernel, vfrac=vfrac, Gc=Gc, keep=keep)
    rho, dp = _f64(rho), _f64(dp)
    _same_side(dev, rho, dp, vstar, p)
    na = int(parts["nall"])
    _need(rho, na, "rho [nall]"); _need(dp, na, "dp [nall]"); _need(vstar, 3 * na, "vstar [nall][3]"); _need(p, na, "p [nall]")
    _check(lib().isph_correct_velocity_pressure(ctx.h, C.byref(pv), int(antisym), float(dt), _ptr(rho), _ptr(dp),
                                                _ptr(vstar), _ptr(p), int(incremental), dev))


def advance_begin(ctx, parts, colmap, dt, p, v, vnp1, vfrac, antisym=True, Gc=None, kernel="wendland"):
    keep = []
    pv, dev, keep = particles_view(parts, colmap, kernel=kernel, vfrac=vfrac, Gc=Gc, keep=keep)
    p, v, vnp1 = _f64(p), _f64(v), _f64(vnp1)
    _same_side(dev, p, v, vnp1)
    na = int(parts["nall"])
    _need(p, na, "p [nall]"); _need(v, 3 * na, "v [nall][3]"); _need(vnp1, 3 * na, "vnp1 [nall][3]")
    out = _out_like(dev, p, (int(parts["nlocal"]),))
    _check(lib().isph_advance_begin(ctx.h, C.byref(pv), int(antisym), float(dt), _ptr(p), _ptr(v), _ptr(vnp1), _ptr(out),
                                    dev))
    return out


def advance_end(ctx, count, dim, dt, dp, vnp1, p, x, v):
    """in-place on p [count], x [count,3], v [count,3] (all numpy or all device tensors)."""
    dp, vnp1 = _f64(dp), _f64(vnp1)
    dev = int(bool(_is_torch(p)))
    _same_side(dev, dp, vnp1, p, x, v)
    _check(lib().isph_advance_end(ctx.h, int(count), int(dim), float(dt), _ptr(dp), _ptr(vnp1), _ptr(p), _ptr(x),
                                  _ptr(v), dev))


def compute_shift(ctx, parts, colmap, alpha, shiftcut, nonfluidweight, kernel="wendland", kinds=None):
    """isph_compute_shift -> dr [nlocal, 3]."""
    keep = []
    if _is_torch(parts["x"]):
        import torch
        ones = torch.ones(int(parts["nall"]), dtype=torch.float64, device=parts["x"].device)
    else:
        ones = np.ones(int(parts["nall"]))
    pv, dev, keep = particles_view(parts, colmap, kernel=kernel, vfrac=ones, keep=keep, kinds=kinds)
    dr = _out_like(dev, parts["x"], (int(parts["nlocal"]), 3))
    _check(lib().isph_compute_shift(ctx.h, C.byref(pv), float(alpha), float(shiftcut), float(nonfluidweight), _ptr(dr),
                                    dev))
    return dr


def apply_shift(ctx, parts, colmap, dr, x, v, p, vfrac, antisym=True, fixed=None, Gc=None, kernel="wendland", kinds=None):
    """isph_apply_shift: in place on x, v [nall,3] and p [nall] (numpy)."""
    keep = []
    pv, dev, keep = particles_view(parts, colmap, kernel=kernel, vfrac=vfrac, Gc=Gc, keep=keep, kinds=kinds)
    fx = None if fixed is None else np.ascontiguousarray(fixed, dtype=np.int32)
    dr = _f64(dr)
    _same_side(dev, dr, x, v, p)
    na = int(parts["nall"])
    _need(dr, 3 * int(parts["nlocal"]), "dr [nlocal][3]"); _need(x, 3 * na, "x [nall][3]"); _need(v, 3 * na, "v [nall][3]"); _need(p, na, "p [nall]")
    _check(lib().isph_apply_shift(ctx.h, C.byref(pv), int(antisym), _ptr(fx), _ptr(dr), _ptr(x), _ptr(v), _ptr(p), dev))


def shift_particles(ctx, parts, colmap, shift, shiftcut, nonfluidweight, dt, x, v, p, vfrac, antisym=True, fixed=None,
                    Gc=None, kernel="wendland", kinds=None):
    """isph_shift_particles: in place on x, v, p; returns the max fluid speed used."""
    keep = []
    pv, dev, keep = particles_view(parts, colmap, kernel=kernel, vfrac=vfrac, Gc=Gc, keep=keep, kinds=kinds)
    fx = None if fixed is None else np.ascontiguousarray(fixed, dtype=np.int32)
    vmax = C.c_double(0.0)
    _same_side(dev, x, v, p)
    na = int(parts["nall"])
    _need(x, 3 * na, "x [nall][3]"); _need(v, 3 * na, "v [nall][3]"); _need(p, na, "p [nall]")
    _check(lib().isph_shift_particles(ctx.h, C.byref(pv), int(antisym), _ptr(fx), float(shift), float(shiftcut),
                                      float(nonfluidweight), float(dt), _ptr(x), _ptr(v), _ptr(p), C.byref(vmax), dev))
    return vmax.value


# ---- two-phase flow: wall normals and surface tension --------------------------------------------------------------

CSF_COLORS = {"corrected": 0, "adami": 1}
PAIRWISE_MODELS = {"tartakovsky-meakin": 0, "tartakovsky-panchenko-var1": 1, "tartakovsky-panchenko-var2": 2}


class _CsfParams(C.Structure):
    _fields_ = [("color", C.c_int), ("alpha", C.c_double), ("theta", C.c_double), ("epsilon", C.c_double),
                ("kappa", C.c_double), ("phase", C.c_void_p)]


class CsfParams:
    """isph_csf_params == st.csf of the reference (pair_isph.cpp:1583-1586): color "corrected" | "adami", alpha, theta,
    epsilon, kappa (defaults 1, 0, 0.01, 100) and phase, the phase of every particle type (phase[t - 1] for type t;
    solids 0)."""

    def __init__(self, phase, color="corrected", alpha=1.0, theta=0.0, epsilon=0.01, kappa=100.0):
        self.phase = np.ascontiguousarray([0] + [int(q) for q in phase], dtype=np.int32)
        self.color = CSF_COLORS[color] if isinstance(color, str) else int(color)
        self.alpha, self.theta, self.epsilon, self.kappa = float(alpha), float(theta), float(epsilon), float(kappa)

    def c_struct(self, ntypes):
        """the C view; the phase table must cover the particle view's types"""
        _need(self.phase, ntypes + 1, "phase [ntypes+1]")
        return _CsfParams(self.color, self.alpha, self.theta, self.epsilon, self.kappa, _ptr(self.phase))


def compute_normals(ctx, parts, colmap, vfrac, Gc, kernel="wendland", kinds=None, with_pnd=True):
    """isph_compute_normals == PairISPH_Corrected::computeNormals (Solid walls): (normal [nlocal, 3], pnd [nlocal]) or
    the normals alone with with_pnd=False."""
    keep = []
    pv, dev, keep = particles_view(parts, colmap, kernel=kernel, vfrac=vfrac, Gc=Gc, keep=keep, kinds=kinds)
    if Gc is None or vfrac is None:
        raise IsphError("compute_normals needs vfrac and Gc")
    n = int(parts["nlocal"])
    nrm = _out_like(dev, parts["x"], (n, 3))
    pnd = _out_like(dev, parts["x"], (n,)) if with_pnd else None
    _check(lib().isph_compute_normals(ctx.h, C.byref(pv), _ptr(nrm), _ptr(pnd), dev))
    return (nrm, pnd) if with_pnd else nrm


def _csf_view(parts, colmap, prm, vfrac, Gc, kernel, kinds, pnd, rho, wall_normal):
    if Gc is None or vfrac is None:
        raise IsphError("the continuum surface force needs vfrac and Gc")
    if wall_normal is not None and pnd is None:
        raise IsphError("the contact-angle correction needs pnd")
    keep = []
    pv, dev, keep = particles_view(parts, colmap, kernel=kernel, vfrac=vfrac, Gc=Gc, keep=keep, kinds=kinds, pnd=pnd)
    rho = None if rho is None else _f64(rho)
    wall_normal = None if wall_normal is None else _f64(wall_normal)
    _same_side(dev, rho, wall_normal)
    _need(rho, int(parts["nall"]), "rho [nall]")
    _need(wall_normal, 3 * int(parts["nlocal"]), "wall_normal [nlocal][3]")
    cp = prm.c_struct(pv.ntypes)
    keep += [prm, cp, rho, wall_normal]
    return pv, dev, keep, cp, rho, wall_normal


def csf_phase_normal(ctx, parts, colmap, prm, vfrac, Gc, rho=None, wall_normal=None, pnd=None, kernel="wendland",
                     kinds=None, with_grad=True):
    """isph_csf_phase_normal: (grad [nlocal, 3] or None, nmag [nlocal, 4] = unit phase normal and |grad c|)."""
    pv, dev, keep, cp, rho, wall_normal = _csf_view(parts, colmap, prm, vfrac, Gc, kernel, kinds, pnd, rho, wall_normal)
    n = int(parts["nlocal"])
    grad = _out_like(dev, parts["x"], (n, 3)) if with_grad else None
    nmag = _out_like(dev, parts["x"], (n, 4))
    _check(lib().isph_csf_phase_normal(ctx.h, C.byref(pv), C.byref(cp), _ptr(rho), _ptr(wall_normal), _ptr(grad),
                                       _ptr(nmag), dev))
    return grad, nmag


def csf_force(ctx, parts, colmap, prm, vfrac, Gc, nmag, f, kernel="wendland", kinds=None, with_kappa=True):
    """isph_csf_force: f [nlocal, 3] is incremented in place; nmag [nall, 4] with the ghost records filled.  Returns the
    curvature [nlocal] (None with with_kappa=False)."""
    pv, dev, keep, cp, _, _ = _csf_view(parts, colmap, prm, vfrac, Gc, kernel, kinds, None, None, None)
    nmag = _f64(nmag)
    _same_side(dev, nmag, f)
    n = int(parts["nlocal"])
    _need(nmag, 4 * int(parts["nall"]), "nmag [nall][4]"); _need(f, 3 * n, "f [nlocal][3]")
    kap = _out_like(dev, parts["x"], (n,)) if with_kappa else None
    _check(lib().isph_csf_force(ctx.h, C.byref(pv), C.byref(cp), _ptr(nmag), _ptr(f), _ptr(kap), dev))
    return kap


def surface_tension_csf(ctx, parts, colmap, prm, vfrac, Gc, f, rho=None, wall_normal=None, pnd=None, plan=None,
                        kernel="wendland", kinds=None, with_nmag=False):
    """isph_surface_tension_csf: both sweeps; f [nlocal, 3] incremented in place.  plan: a HaloForward for the off-rank
    ghosts (None on one rank).  Returns nmag [nlocal, 4] with with_nmag=True."""
    pv, dev, keep, cp, rho, wall_normal = _csf_view(parts, colmap, prm, vfrac, Gc, kernel, kinds, pnd, rho, wall_normal)
    _same_side(dev, f)
    n = int(parts["nlocal"])
    _need(f, 3 * n, "f [nlocal][3]")
    nmag = _out_like(dev, parts["x"], (n, 4)) if with_nmag else None
    _check(lib().isph_surface_tension_csf(ctx.h, C.byref(pv), C.byref(cp), None if plan is None else plan.h, _ptr(rho),
                                          _ptr(wall_normal), _ptr(f), _ptr(nmag), dev))
    return nmag


def pairwise_force(ctx, parts, colmap, model, phase, s, f, kernel="wendland", kinds=None):
    """isph_pairwise_force: f [nlocal, 3] incremented in place; phase as in CsfParams; s [nphase, nphase].  Returns the
    sum of the added forces (the functor's _f_sum)."""
    keep = []
    pv, dev, keep = particles_view(parts, colmap, kernel=kernel, keep=keep, kinds=kinds)
    ph = np.ascontiguousarray([0] + [int(q) for q in phase], dtype=np.int32)
    s = np.ascontiguousarray(s, dtype=np.float64)
    if s.ndim != 2 or s.shape[0] != s.shape[1]:
        raise OperandError("s must be [nphase][nphase]")
    nphase = int(s.shape[0])
    _same_side(dev, f)
    _need(ph, pv.ntypes + 1, "phase [ntypes+1]"); _need(f, 3 * int(parts["nlocal"]), "f [nlocal][3]")
    if ph.min() < 0 or ph.max() >= nphase:
        raise OperandError("phase outside [0, nphase)")
    fsum = np.zeros(3)
    m = PAIRWISE_MODELS[model] if isinstance(model, str) else int(model)
    _check(lib().isph_pairwise_force(ctx.h, C.byref(pv), m, _ptr(ph), _ptr(s), nphase, _ptr(f), _ptr(fsum), dev))
    return fsum


# ---- body forces: electrostatic force and random stress -------------------------------------------------------------

def smooth_field(ctx, parts, colmap, f, vfrac, filt=None, out=None, kernel="wendland", kinds=None):
    """isph_smooth_field == FunctorOuterSmoothField, one pass: f [nall] -> sf [nlocal].  filt = (filt_i, filt_j) or None;
    rows whose kind fails filt_i are not written: they keep what `out` holds (zeros when out is None)."""
    if vfrac is None:
        raise OperandError("smooth_field needs vfrac [nall]")
    keep = []
    pv, dev, keep = particles_view(parts, colmap, kernel=kernel, vfrac=vfrac, keep=keep, kinds=kinds)
    f = _f64(f)
    _same_side(dev, f, out)
    n = int(parts["nlocal"])
    _need(f, int(parts["nall"]), "f [nall]")
    if out is None:
        out = _out_like(dev, f, (n,))
    _need(out, n, "sf_out [nlocal]")
    fi, fj = filt if filt is not None else (127, 127)
    _check(lib().isph_smooth_field(ctx.h, C.byref(pv), _ptr(f), int(filt is not None), int(fi), int(fj), _ptr(out), dev))
    return out


class EkParams(C.Structure):
    """isph_ek_params: pb.ezcb, pb.psiref, pb.gamma (defaults 0, 1, 0: pair_isph.cpp:1684-1698), pb_e = pb.e (the field
    used without phi) and ae_e = ae.e (phigrad = -ae_e on the buffer rows)."""
    _fields_ = [("ezcb", C.c_double), ("psiref", C.c_double), ("gamma", C.c_double), ("pb_e", C.c_double * 3),
                ("ae_e", C.c_double * 3)]

    def __init__(self, ezcb=0.0, psiref=1.0, gamma=0.0, pb_e=(0.0, 0.0, 0.0), ae_e=(0.0, 0.0, 0.0)):
        super().__init__(float(ezcb), float(psiref), float(gamma), (C.c_double * 3)(*[float(v) for v in pb_e]),
                         (C.c_double * 3)(*[float(v) for v in ae_e]))


def electrostatic_force(ctx, parts, colmap, prm, psi, vfrac, phi=None, f=None, antisym=False, Gc=None, pnd=None,
                        morris_holmes=None, morris_safe_coeff=0.43301, kernel="wendland", kinds=None, with_gradients=True):
    """isph_electrostatic_force: the psi gradient (Fluid, All; MorrisHolmes mirror when pnd is given), the phi gradient
    (Fluid, Fluid; -ae_e on the buffer rows) and the force in one sweep.  psi, phi [nall]; f [nlocal, 3] is incremented
    in place (None: gradients only).  morris_holmes: None = mirrored exactly when pnd is given.  Returns (psigrad,
    phigrad), each [nlocal, 3] (phigrad None without phi), or None with with_gradients=False."""
    if vfrac is None:
        raise OperandError("electrostatic_force needs vfrac [nall]")
    if morris_holmes is None:
        morris_holmes = pnd is not None
    if morris_holmes and pnd is None:
        raise OperandError("the MorrisHolmes mirror needs pnd [nall]")
    if not morris_holmes:
        pnd = None
    if not antisym and Gc is None:
        raise OperandError("the Symmetric gradient (antisym = 0) needs Gc")
    keep = []
    pv, dev, keep = particles_view(parts, colmap, kernel=kernel, vfrac=vfrac, Gc=Gc, keep=keep, kinds=kinds, pnd=pnd,
                                   morris_safe_coeff=morris_safe_coeff)
    psi = _f64(psi)
    phi = None if phi is None else _f64(phi)
    _same_side(dev, psi, phi, f)
    n, na = int(parts["nlocal"]), int(parts["nall"])
    _need(psi, na, "psi [nall]"); _need(phi, na, "phi [nall]"); _need(f, 3 * n, "f [nlocal][3]")
    gpsi = _out_like(dev, psi, (n, 3)) if with_gradients else None
    gphi = _out_like(dev, psi, (n, 3)) if with_gradients and phi is not None else None
    _check(lib().isph_electrostatic_force(ctx.h, C.byref(pv), int(antisym), C.byref(prm), _ptr(psi), _ptr(phi), _ptr(gpsi),
                                          _ptr(gphi), _ptr(f), dev))
    return (gpsi, gphi) if with_gradients else None


def _rs_view(parts, colmap, vfrac, kernel, kinds):
    if vfrac is None:
        raise OperandError("the random stress needs vfrac [nall]")
    keep = []
    return particles_view(parts, colmap, kernel=kernel, vfrac=vfrac, keep=keep, kinds=kinds)


def random_stress_tensor(ctx, parts, colmap, tag, seed, step, kernel="wendland", kinds=None):
    """isph_random_stress_tensor: rs [nlocal, 6], the traceless symmetric tensor of every Fluid particle packed as (0,0),
    (0,1), (1,1), (0,2), (1,2), (2,2); a function of (seed, step, tag) alone (Philox4x32-10)."""
    keep = []
    pv, dev, keep = particles_view(parts, colmap, kernel=kernel, keep=keep, kinds=kinds)
    tag = _i32(tag)
    _same_side(dev, tag)
    n = int(parts["nlocal"])
    _need(tag, n, "tag [nlocal]")
    rs = _out_like(dev, parts["x"], (n, 6))
    _check(lib().isph_random_stress_tensor(ctx.h, C.byref(pv), _ptr(tag), int(seed), int(step), _ptr(rs), dev))
    return rs


def random_stress_force(ctx, parts, colmap, dt, kBT, nu, rho, rs, f, vfrac, kernel="wendland", kinds=None):
    """isph_random_stress_force: f [nlocal, 3] incremented in place on the Fluid rows; rs [nall, 6] with the ghost records
    filled; nu, rho [nlocal]."""
    pv, dev, keep = _rs_view(parts, colmap, vfrac, kernel, kinds)
    nu, rho, rs = _f64(nu), _f64(rho), _f64(rs)
    _same_side(dev, nu, rho, rs, f)
    n = int(parts["nlocal"])
    _need(nu, n, "nu [nlocal]"); _need(rho, n, "rho [nlocal]"); _need(rs, 6 * int(parts["nall"]), "rs [nall][6]")
    _need(f, 3 * n, "f [nlocal][3]")
    _check(lib().isph_random_stress_force(ctx.h, C.byref(pv), float(dt), float(kBT), _ptr(nu), _ptr(rho), _ptr(rs), _ptr(f), dev))


def force_from_random_stress(ctx, parts, colmap, tag, seed, step, dt, kBT, nu, rho, f, vfrac, plan=None, kernel="wendland",
                             kinds=None, with_rs=False):
    """isph_force_from_random_stress: tensors, ghost fill (through colmap; plan: a HaloForward for the off-rank ghosts) and
    the sweep in one call; f [nlocal, 3] incremented in place.  Returns rs [nlocal, 6] with with_rs=True."""
    pv, dev, keep = _rs_view(parts, colmap, vfrac, kernel, kinds)
    tag, nu, rho = _i32(tag), _f64(nu), _f64(rho)
    _same_side(dev, tag, nu, rho, f)
    n = int(parts["nlocal"])
    _need(tag, n, "tag [nlocal]"); _need(nu, n, "nu [nlocal]"); _need(rho, n, "rho [nlocal]"); _need(f, 3 * n, "f [nlocal][3]")
    rs = _out_like(dev, parts["x"], (n, 6)) if with_rs else None
    _check(lib().isph_force_from_random_stress(ctx.h, C.byref(pv), None if plan is None else plan.h, _ptr(tag), int(seed),
                                               int(step), float(dt), float(kBT), _ptr(nu), _ptr(rho), _ptr(f), _ptr(rs), dev))
    return rs


class NeighbourList:
    """isph_nlist: ghost atoms (periodic images) and the full neighbour list of one rank's owned particles, built on the
    device (isph_nlist_build) -- the device twin of workload.make_cloud.  x [nlocal, 3]: a numpy array or a torch device
    tensor; the outputs of get() live on the same side.  lo / hi / periodic: the box, `dim` entries each (or three).
    Raises ValueError before any library call for a wrong x shape, cut <= 0 or a periodic axis shorter than two cuts."""

    def __init__(self, ctx, x, lo, hi, periodic, cut, dim, wrap=True):
        self.h = C.c_void_p()
        self.ctx = ctx
        if dim not in (2, 3):
            raise ValueError("dim must be 2 or 3")
        if len(x.shape) != 2 or int(x.shape[1]) != 3:
            raise ValueError("x must be [nlocal, 3], got %s" % (tuple(x.shape),))
        if not float(cut) > 0.0:
            raise ValueError("cut must be positive")
        lo3 = [float(v) for v in (list(lo) + [0.0] * 3)[:3]]
        hi3 = [float(v) for v in (list(hi) + [1.0] * 3)[:3]]
        per3 = [int(bool(v)) for v in (list(periodic) + [0] * 3)[:3]]
        for a in range(dim):
            if per3[a] and hi3[a] - lo3[a] < 2.0 * float(cut):
                raise ValueError("periodic axis %d is shorter than two cuts" % a)
        x = _f64(x)
        if _is_torch(x) and not x.is_contiguous():
            x = x.contiguous()
        self.dev = _on_device(x)
        self._like = x
        self.dim, self.nlocal = dim, int(x.shape[0])
        _check(lib().isph_nlist_build(ctx.h, dim, self.nlocal, _ptr(x), (C.c_double * 3)(*lo3), (C.c_double * 3)(*hi3),
                                      (C.c_int * 3)(*per3), float(cut), int(bool(wrap)), self.dev, C.byref(self.h)))

    @property
    def info(self):
        """dict(nlocal, nghost, entries, fits32)"""
        a = (C.c_longlong * 4)()
        _check(lib().isph_nlist_info(self.h, a))
        return dict(nlocal=int(a[0]), nghost=int(a[1]), entries=int(a[2]), fits32=int(a[3]))

    def _empty(self, shape, kind):
        if self.dev:
            import torch
            return torch.empty(shape, dtype=getattr(torch, kind), device=self._like.device)
        return np.empty(shape, dtype=getattr(np, kind))

    def get(self, ptr64=False):
        """dict(x [nall, 3], owner_index [nall], neigh_ptr [nlocal + 1], neigh_idx [entries]).  neigh_ptr is int32 while
        the entries fit (the rule of workload.make_cloud) unless ptr64 is set, else int64."""
        i = self.info
        nall = i["nlocal"] + i["nghost"]
        wide = bool(ptr64) or not i["fits32"]
        x, own = self._empty((nall, 3), "float64"), self._empty((nall,), "int32")
        nptr = self._empty((i["nlocal"] + 1,), "int64" if wide else "int32")
        nidx = self._empty((i["entries"],), "int32")
        _check(lib().isph_nlist_get(self.ctx.h, self.h, _ptr(x), _ptr(own), _ptr(nptr) if wide else None,
                                    None if wide else _ptr(nptr), _ptr(nidx), self.dev))
        return dict(x=x, owner_index=own, neigh_ptr=nptr, neigh_idx=nidx)

    def close(self):
        if self.h:
            lib().isph_nlist_destroy(self.ctx.h, self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _CDecomp(C.Structure):
    _fields_ = [("dim", C.c_int), ("lo", C.c_double * 3), ("hi", C.c_double * 3), ("periodic", C.c_int * 3),
                ("pgrid", C.c_int * 3), ("faces", C.c_void_p * 3)]


class _FwdArray(C.Structure):
    _fields_ = [("a", C.c_void_p), ("ncomp", C.c_int), ("is_int", C.c_int)]


class Decomp:
    """isph_decomp: a brick of pgrid[0] x pgrid[1] x pgrid[2] ranks over the box lo .. hi (`dim` entries each, or three);
    rank = cx + pgrid[0] * (cy + pgrid[1] * cz).  faces: None (uniform cuts) or per axis None / the pgrid[a] + 1 cut planes
    from lo to hi.  Grid cell c owns x when faces[c] <= x < faces[c + 1]."""

    def __init__(self, dim, lo, hi, periodic, pgrid, faces=None):
        if dim not in (2, 3):
            raise ValueError("dim must be 2 or 3")
        self.dim = int(dim)
        self.lo = [float(v) for v in (list(lo) + [0.0] * 3)[:3]]
        self.hi = [float(v) for v in (list(hi) + [0.0] * 3)[:3]]
        self.periodic = [int(bool(v)) for v in (list(periodic) + [0] * 3)[:3]]
        self.pgrid = [int(v) for v in (list(pgrid) + [1] * 3)[:3]]
        for a in range(self.dim, 3):
            self.lo[a], self.hi[a], self.periodic[a], self.pgrid[a] = 0.0, 0.0, 0, 1
        self.faces = [None, None, None]
        for a in range(self.dim):
            if faces is not None and faces[a] is not None:
                f = np.ascontiguousarray(faces[a], dtype=np.float64)
                if f.shape != (self.pgrid[a] + 1,):
                    raise ValueError("faces[%d]: pgrid[%d] + 1 = %d planes needed" % (a, a, self.pgrid[a] + 1))
                self.faces[a] = f

    @property
    def nranks(self):
        return self.pgrid[0] * self.pgrid[1] * self.pgrid[2]

    def c_struct(self):
        """the isph_decomp; it points into self.faces: keep self alive for the duration of the call"""
        d = _CDecomp()
        d.dim = self.dim
        for a in range(3):
            d.lo[a], d.hi[a], d.periodic[a], d.pgrid[a] = self.lo[a], self.hi[a], self.periodic[a], self.pgrid[a]
            d.faces[a] = None if self.faces[a] is None else self.faces[a].ctypes.data
        return d


class NeighbourListDist(NeighbourList):
    """isph_nlist_build_dist: ghost atoms from the neighbouring ranks and from periodic images, the full list, the column
    map and the halo plan of this rank's owned particles x [nlocal, 3] (numpy or torch device tensor; nlocal = 0 takes
    part), built on the device.  COLLECTIVE: every rank of the context constructs one, with the same decomp, cut and prune.
    get() adds owner_rank and colmap; plan() is the dist.HaloPlan Matrix.set_halo / HaloForward take; forward() is
    forward_comm_pair of a per-atom array through that plan."""

    def __init__(self, ctx, x, decomp, cut, prune=True):
        self.h = C.c_void_p()
        self.ctx, self.decomp = ctx, decomp
        if len(x.shape) != 2 or int(x.shape[1]) != 3:
            raise ValueError("x must be [nlocal, 3], got %s" % (tuple(x.shape),))
        x = _f64(x)
        if _is_torch(x) and not x.is_contiguous():
            x = x.contiguous()
        self.dev = _on_device(x)
        self._like = x
        self.dim, self.nlocal = decomp.dim, int(x.shape[0])
        cd = decomp.c_struct()
        _check(lib().isph_nlist_build_dist(ctx.h, C.byref(cd), self.nlocal, _ptr(x) if self.nlocal else None, float(cut),
                                           int(bool(prune)), self.dev, C.byref(self.h)))

    @property
    def info(self):
        """dict(nlocal, nghost, entries, fits32, ncol, npeers, nsend, noffrank)"""
        a = (C.c_longlong * 8)()
        _check(lib().isph_nlist_dist_info(self.h, a))
        return dict(nlocal=int(a[0]), nghost=int(a[1]), entries=int(a[2]), fits32=int(a[3]), ncol=int(a[4]), npeers=int(a[5]),
                    nsend=int(a[6]), noffrank=int(a[7]))

    def get(self, ptr64=False):
        """NeighbourList.get() + owner_rank [nall], colmap [nall] (on the side of x)"""
        g = NeighbourList.get(self, ptr64)
        i = self.info
        nall = i["nlocal"] + i["nghost"]
        orank, colmap = self._empty((nall,), "int32"), self._empty((nall,), "int32")
        _check(lib().isph_nlist_dist_get(self.ctx.h, self.h, _ptr(orank), _ptr(colmap), None, None, None, None, self.dev))
        g.update(owner_rank=orank, colmap=colmap)
        return g

    def plan(self):
        """dist.HaloPlan of the list (numpy arrays on the host)"""
        from . import dist
        i = self.info
        n, nall, npeers = i["nlocal"], i["nlocal"] + i["nghost"], i["npeers"]
        orank, colmap, own = (np.zeros(nall, dtype=np.int32) for _ in range(3))
        peers, sp, rp = np.zeros(npeers, dtype=np.int32), np.zeros(npeers + 1, dtype=np.int32), np.zeros(npeers + 1, dtype=np.int32)
        sidx = np.zeros(i["nsend"], dtype=np.int32)
        _check(lib().isph_nlist_dist_get(self.ctx.h, self.h, _ptr(orank), _ptr(colmap), _ptr(peers), _ptr(sp), _ptr(sidx), _ptr(rp), 0))
        _check(lib().isph_nlist_get(self.ctx.h, self.h, None, _ptr(own), None, None, None, 0))
        p = dist.HaloPlan(int(self.ctx.rank), int(self.ctx.nranks), n, i["ncol"], colmap, peers, sp, sidx, rp)
        p.ghost_col_of = colmap[n:].copy()
        ridx = np.zeros(i["ncol"] - n, dtype=np.int32)
        off = colmap >= n
        ridx[colmap[off] - n] = own[off]
        p.recv_idx = ridx
        return p

    def forward(self, a, ncomp=None):
        """isph_nlist_forward / _forward_int, in place: rows >= nlocal of a [nall] or [nall, ncomp] (float64 or int32, C
        contiguous, numpy or device tensor) receive their owner's row.  Collective.  Returns a."""
        i = self.info
        nall = i["nlocal"] + i["nghost"]
        if a.ndim not in (1, 2) or int(a.shape[0]) != nall:
            raise OperandError("a: %s given, [nall = %d] or [nall][ncomp] needed" % (tuple(a.shape), nall))
        nc = 1 if a.ndim == 1 else int(a.shape[1])
        if ncomp is not None and int(ncomp) != nc:
            raise OperandError("a has %d components, ncomp = %d" % (nc, int(ncomp)))
        if nc < 1:
            raise OperandError("a needs at least one component")
        kind = str(a.dtype).replace("torch.", "")
        if kind not in ("float64", "int32"):
            raise ValueError("a: float64 or int32 needed, got %s" % a.dtype)
        if (_is_torch(a) and not a.is_contiguous()) or (not _is_torch(a) and not a.flags.c_contiguous):
            raise ValueError("a: a C-contiguous array is updated in place")
        fn = lib().isph_nlist_forward if kind == "float64" else lib().isph_nlist_forward_int
        _check(fn(self.ctx.h, self.h, nc, _ptr(a) if nall else None, _on_device(a)))
        return a

    def forward_multi(self, arrays):
        """isph_nlist_forward_multi: the forward of up to 8 arrays ([nall] or [nall, ncomp], float64 or int32, C contiguous,
        all numpy or all device tensors) in ONE exchange, in place.  Collective.  Returns the list."""
        arrays = list(arrays)
        if not 1 <= len(arrays) <= 8:
            raise OperandError("forward_multi takes 1 to 8 arrays, %d given" % len(arrays))
        i = self.info
        nall = i["nlocal"] + i["nghost"]
        rec = (_FwdArray * len(arrays))()
        for j, a in enumerate(arrays):
            if a.ndim not in (1, 2) or int(a.shape[0]) != nall:
                raise OperandError("array %d: %s given, [nall = %d] or [nall][ncomp] needed" % (j, tuple(a.shape), nall))
            kind = str(a.dtype).replace("torch.", "")
            if kind not in ("float64", "int32"):
                raise ValueError("array %d: float64 or int32 needed, got %s" % (j, a.dtype))
            if (_is_torch(a) and not a.is_contiguous()) or (not _is_torch(a) and not a.flags.c_contiguous):
                raise ValueError("array %d: a C-contiguous array is updated in place" % j)
            nc = 1 if a.ndim == 1 else int(a.shape[1])
            if nc < 1:
                raise OperandError("array %d needs at least one component" % j)
            rec[j].a, rec[j].ncomp, rec[j].is_int = (_ptr(a) if nall else None), nc, int(kind == "int32")
        _check(lib().isph_nlist_forward_multi(self.ctx.h, self.h, len(arrays), rec, _on_device(*arrays)))
        return arrays


def migrate(ctx, decomp, x, fd=None, fi=None):
    """isph_migrate (Comm::exchange): x [nlocal, 3] is wrapped and every particle goes to the rank whose sub-box holds it,
    with its row of fd [nlocal, nd] (float64) and fi [nlocal, ni] (int32).  COLLECTIVE.  Returns (x, fd, fi, info) on the
    side of x: the stayers in their old order, then the arrivals by (source rank, source index); info = dict(nlocal, sent,
    received).  fd / fi None: returned as [nlocal', 0]."""
    x = _f64(x)
    n = int(x.shape[0])
    if len(x.shape) != 2 or int(x.shape[1]) != 3:
        raise ValueError("x must be [nlocal, 3], got %s" % (tuple(x.shape),))
    dev = _on_device(x)
    nd = 0 if fd is None else int(fd.shape[1])
    ni = 0 if fi is None else int(fi.shape[1])
    if fd is not None:
        fd = _f64(fd)
        if fd.ndim != 2 or int(fd.shape[0]) != n:
            raise OperandError("fd: [nlocal = %d][nd] needed" % n)
        _same_side(dev, fd)
    if fi is not None:
        fi = _i32(fi)
        if fi.ndim != 2 or int(fi.shape[0]) != n:
            raise OperandError("fi: [nlocal = %d][ni] needed" % n)
        _same_side(dev, fi)
    for a in (x, fd, fi):
        if a is not None and _is_torch(a) and not a.is_contiguous():
            raise ValueError("contiguous tensors needed")
    h = C.c_void_p()
    cd = decomp.c_struct()
    _check(lib().isph_migrate(ctx.h, C.byref(cd), n, _ptr(x) if n else None, nd, _ptr(fd) if n and nd else None, ni,
                              _ptr(fi) if n and ni else None, dev, C.byref(h)))
    try:
        a = (C.c_longlong * 3)()
        _check(lib().isph_migrated_info(h, a))
        m = int(a[0])

        def empty(shape, kind):
            if dev:
                import torch
                return torch.empty(shape, dtype=getattr(torch, kind), device=x.device)
            return np.empty(shape, dtype=getattr(np, kind))
        xo, fdo, fio = empty((m, 3), "float64"), empty((m, nd), "float64"), empty((m, ni), "int32")
        _check(lib().isph_migrated_get(ctx.h, h, _ptr(xo) if m else None, _ptr(fdo) if m and nd else None,
                                       _ptr(fio) if m and ni else None, dev))
    finally:
        lib().isph_migrated_destroy(ctx.h, h)
    return xo, fdo, fio, dict(nlocal=m, sent=int(a[1]), received=int(a[2]))


# ---- the glue of a time step: ghost rows, zero-mean pressure, observables -------------------------------------------

KIND_FLUID, KIND_SOLID, KIND_BUFFER_DIRICHLET, KIND_BUFFER_NEUMANN = 99, 12, 32, 64


def ghost_fill(ctx, nlocal, owner, a):
    """isph_ghost_fill: rows i >= nlocal of a [nall] or [nall, ncomp] receive row owner[i], in place (numpy or device
    tensor, owner on the same side).  nall is len(owner)."""
    owner = _i32(owner)
    nlocal = int(nlocal)
    nall = int(owner.numel()) if _is_torch(owner) else int(owner.size)
    if not _is_torch(a) and not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous):
        raise ValueError("a: a C-contiguous float64 array is updated in place")
    _f64(a)
    dev = _on_device(owner, a)
    if not 0 <= nlocal <= nall:
        raise OperandError("nlocal = %d outside [0, nall = %d]" % (nlocal, nall))
    if a.ndim not in (1, 2) or (nall > 0 and int(a.shape[0]) != nall):
        raise OperandError("a: %s given, [nall = %d] or [nall][ncomp] needed" % (tuple(a.shape), nall))
    ncomp = 1 if a.ndim == 1 else int(a.shape[1])
    _need(a, nall * ncomp, "a [nall][ncomp]")
    _check(lib().isph_ghost_fill(ctx.h if ctx is not None else None, nlocal, nall, _ptr(owner), ncomp, _ptr(a), dev))
    return a


def _zero_mean_call(fn, ctx, nlocal, type, kinds, f, update, want_mean):
    """the operand checks and the call isph_zero_mean_pressure and its _dist form share"""
    typ = _i32(type)
    nall = int(typ.numel()) if _is_torch(typ) else int(typ.size)
    nlocal = int(nlocal)
    if kinds is None:
        ntypes = 1 if nall == 0 else (int(typ.max().item()) if _is_torch(typ) else int(np.max(typ)))
        kinds = [KIND_FLUID] * ntypes
    ntypes = len(kinds)
    kind = np.ascontiguousarray([0] + list(kinds), dtype=np.int32)
    if not _is_torch(f) and not (isinstance(f, np.ndarray) and f.dtype == np.float64 and f.flags.c_contiguous):
        raise ValueError("f: a C-contiguous float64 array is updated in place")
    _f64(f)
    dev = _on_device(typ, f)
    if not 0 <= nlocal <= nall:
        raise OperandError("nlocal = %d outside [0, nall = %d]" % (nlocal, nall))
    _need(f, nall, "f [nall]")
    mean = C.c_double(0.0)
    _check(fn(ctx.h if ctx is not None else None, nlocal, nall, _ptr(typ), _ptr(kind), ntypes, _ptr(f), int(bool(update)),
              C.byref(mean) if want_mean else None, dev))
    return mean.value if want_mean else None


def zero_mean_pressure(ctx, nlocal, type, kinds, f, update=True, want_mean=True):
    """isph_zero_mean_pressure: in place on f [nall] (numpy or device tensor, like type); kinds = the kind of type 1, 2,
    ... as in particles_view (None: all Fluid).  Returns the mean (None when want_mean is False: nothing is read back)."""
    return _zero_mean_call(lib().isph_zero_mean_pressure, ctx, nlocal, type, kinds, f, update, want_mean)


def zero_mean_pressure_dist(ctx, nlocal, type, kinds, f, update=True, want_mean=True):
    """isph_zero_mean_pressure_dist: zero_mean_pressure over the owned rows of ALL ranks of ctx.  COLLECTIVE; pass kinds
    (the table cannot be guessed from one rank's types)."""
    if kinds is None:
        raise ValueError("zero_mean_pressure_dist: kinds is needed")
    return _zero_mean_call(lib().isph_zero_mean_pressure_dist, ctx, nlocal, type, kinds, f, update, want_mean)


STATUS_FIELDS = ("count", "sum_vx", "sum_vy", "sum_vz", "volume", "mass", "kinetic_energy", "vmax")


def _status_call(fn, ctx, nlocal, x, type, vfrac, v, rho, type_mask, centre, radius):
    """the operand checks and the call isph_status and its _dist form share"""
    n = int(nlocal)
    x, v, vfrac, rho, typ = _f64(x), _f64(v), _f64(vfrac), _f64(rho), _i32(type)
    dev = _on_device(x, v, vfrac, rho, typ)
    _need(x, 3 * n, "x [nlocal][3]"); _need(v, 3 * n, "v [nlocal][3]"); _need(vfrac, n, "vfrac [nlocal]")
    _need(rho, n, "rho [nlocal]"); _need(typ, n, "type [nlocal]")
    pv = _Particles()
    pv.dim, pv.nlocal, pv.nall = 3, n, n
    pv.x, pv.type, pv.vfrac = _ptr(x), _ptr(typ), _ptr(vfrac)
    c = (C.c_double * 3)(*[float(t) for t in centre])
    out = (C.c_double * 8)()
    mask = int(type_mask) & 0xFFFFFFFF
    mask = mask - (1 << 32) if mask >= (1 << 31) else mask
    _check(fn(ctx.h if ctx is not None else None, C.byref(pv), mask, _ptr(v), _ptr(rho), c, float(radius), out, dev))
    return np.array(out[:], dtype=np.float64)


def status(ctx, nlocal, x, type, vfrac, v, rho, type_mask=-1, centre=(0.0, 0.0, 0.0), radius=0.0):
    """isph_status == compute isph/status over the owned rows: numpy array of the eight numbers STATUS_FIELDS names.
    x, v [>= nlocal, 3]; type, vfrac, rho [>= nlocal]; all numpy or all device tensors."""
    return _status_call(lib().isph_status, ctx, nlocal, x, type, vfrac, v, rho, type_mask, centre, radius)


def status_dist(ctx, nlocal, x, type, vfrac, v, rho, type_mask=-1, centre=(0.0, 0.0, 0.0), radius=0.0):
    """isph_status_dist: status over the owned rows of ALL ranks of ctx; the same bits on every rank.  COLLECTIVE."""
    return _status_call(lib().isph_status_dist, ctx, nlocal, x, type, vfrac, v, rho, type_mask, centre, radius)


def _tgv_error_call(fn, ctx, nlocal, x, vnp1, p, rho, nu, t, umax, dim):
    """the operand checks and the call isph_tgv_error and its _dist form share"""
    n = int(nlocal)
    x, vnp1, p, rho, nu = _f64(x), _f64(vnp1), _f64(p), _f64(rho), _f64(nu)
    dev = _on_device(x, vnp1, p, rho, nu)
    _need(x, 3 * n, "x [nlocal][3]"); _need(vnp1, 3 * n, "vnp1 [nlocal][3]"); _need(p, n, "p [nlocal]")
    _need(rho, n, "rho [nlocal]"); _need(nu, n, "nu [nlocal]")
    out = (C.c_double * 4)()
    _check(fn(ctx.h if ctx is not None else None, n, int(dim), _ptr(x), _ptr(vnp1), _ptr(p), _ptr(rho), _ptr(nu), float(t),
              float(umax), out, dev))
    return tuple(out[:])


def tgv_error(ctx, nlocal, x, vnp1, p, rho, nu, t, umax, dim=2):
    """isph_tgv_error == the error of fix isph/tgv: (p_err, p_norm, u_err, u_norm).  x, vnp1 [>= nlocal, 3]; p, rho, nu
    [>= nlocal]; all numpy or all device tensors."""
    return _tgv_error_call(lib().isph_tgv_error, ctx, nlocal, x, vnp1, p, rho, nu, t, umax, dim)


def tgv_error_dist(ctx, nlocal, x, vnp1, p, rho, nu, t, umax, dim=2):
    """isph_tgv_error_dist: tgv_error over the owned rows of ALL ranks of ctx; the same bits on every rank.  COLLECTIVE."""
    return _tgv_error_call(lib().isph_tgv_error_dist, ctx, nlocal, x, vnp1, p, rho, nu, t, umax, dim)


# ---- the time step of incompressible Navier-Stokes, resident on the device ------------------------------------------

class _InsParams(C.Structure):
    _fields_ = [("dim", C.c_int), ("kernel", C.c_int), ("antisym", C.c_int), ("theta", C.c_double), ("dt", C.c_double),
                ("incremental_pressure", C.c_int), ("singular_mode", C.c_int), ("g", C.c_double * 3), ("ntypes", C.c_int),
                ("kind", C.c_void_p), ("h", C.c_void_p), ("cutsq", C.c_void_p),
                ("prec_helmholtz", C.c_char_p), ("helmholtz_block_size", C.c_int),
                ("prec_poisson", C.c_char_p), ("poisson_block_size", C.c_int), ("solver", SolverParams),
                ("lo", C.c_double * 3), ("hi", C.c_double * 3), ("periodic", C.c_int * 3), ("cut", C.c_double),
                ("shift", C.c_double), ("shiftcut", C.c_double), ("nonfluidweight", C.c_double),
                ("block_helmholtz", C.c_int), ("morris_holmes", C.c_int), ("normals_bd_coord", C.c_int),
                ("normals_use_part", C.c_int), ("recycle", C.c_void_p), ("tgv_umax", C.c_double),
                ("status_type_mask", C.c_int), ("status_centre", C.c_double * 3), ("status_radius", C.c_double)]


class InsInfo(C.Structure):
    """isph_ins_info: the SolveInfo of the Helmholtz and of the Poisson solve of one step"""
    _fields_ = [("helmholtz", SolveInfo), ("poisson", SolveInfo)]


class InsParams:
    """isph_ins_params.  h and cut are the scalars of the generators (one smoothing length, one pair cut; the tables of
    the ABI are filled with them), kinds the kind of type 1, 2, ... (None: one Fluid type); box = (lo, hi, periodic) and
    list_cut for InsStep.rebuild.  Every other keyword is a field of the struct (theta, dt, antisym, singular_mode,
    incremental_pressure, g, prec_helmholtz, helmholtz_block_size, prec_poisson, poisson_block_size, solver, shift,
    shiftcut, nonfluidweight, tgv_umax, status_type_mask, status_centre, status_radius, and the refused block_helmholtz,
    morris_holmes, normals_bd_coord, normals_use_part, recycle)."""

    def __init__(self, dim, dt, h, cut, kinds=None, kernel="wendland", box=None, list_cut=None, **kw):
        s = self.c = _InsParams()
        lib().isph_ins_params_default(C.byref(s))
        kinds = [KIND_FLUID] if kinds is None else list(kinds)
        nt = len(kinds)
        self._kind = np.ascontiguousarray([0] + kinds, dtype=np.int32)
        self._h = np.full((nt + 1, nt + 1), float(h))
        self._cutsq = np.full((nt + 1, nt + 1), float(cut) ** 2)
        s.dim, s.dt, s.kernel, s.ntypes = int(dim), float(dt), KERNELS[kernel], nt
        s.kind, s.h, s.cutsq = self._kind.ctypes.data, self._h.ctypes.data, self._cutsq.ctypes.data
        if box is not None:
            lo, hi, per = box
            for a in range(3):
                s.lo[a], s.hi[a], s.periodic[a] = float(lo[a]), float(hi[a]), int(per[a])
            s.cut = float(cut if list_cut is None else list_cut)
        for k, v in kw.items():
            if k in ("prec_helmholtz", "prec_poisson"):
                setattr(s, k, v.encode())
            elif k in ("g", "status_centre"):
                for a in range(3):
                    getattr(s, k)[a] = float(v[a])
            elif k == "recycle":
                s.recycle = v.h if hasattr(v, "h") else v
            elif k not in dict(_InsParams._fields_):
                raise TypeError("InsParams: unknown field %r" % k)
            else:
                setattr(s, k, v)


DIAG_FIELDS = ("p_err", "p_norm", "u_err", "u_norm") + STATUS_FIELDS + ("iters_helmholtz", "iters_poisson",
                                                                        "converged_helmholtz", "converged_poisson")
_INS_FIELDS = {"x": (3, np.float64), "v": (3, np.float64), "vstar": (3, np.float64), "f": (3, np.float64),
               "normal": (3, np.float64), "p": (1, np.float64), "dp": (1, np.float64), "rho": (1, np.float64),
               "nu": (1, np.float64), "vfrac": (1, np.float64), "pnd": (1, np.float64), "Gc": (None, np.float64),
               "Lc": (None, np.float64), "type": (1, np.int32), "owner": (1, np.int32), "tag": (1, np.int32),
               "owner_rank": (1, np.int32), "colmap": (1, np.int32)}


class InsStep:
    """isph_ins: one rank's Navier-Stokes state on the device; the methods are the phases of the reference
    (include/isph_hip.h).  Operands are numpy arrays or device tensors.  With decomp (a hip.Decomp) it is the distributed
    driver (isph_ins_create_dist): the state is this rank's share, set_state takes the particles' global ids as tag, and
    every method is COLLECTIVE over the ranks of ctx.  With decomp=None nothing changes."""

    def __init__(self, ctx, params, decomp=None):
        L = lib()
        self.ctx, self.params, self.dim, self.decomp = ctx, params, int(params.c.dim), decomp
        self.h = C.c_void_p()
        if decomp is None:
            _check(L.isph_ins_create(ctx.h, C.byref(params.c), C.byref(self.h)))
        else:
            cd = decomp.c_struct()
            _check(L.isph_ins_create_dist(ctx.h, C.byref(params.c), C.byref(cd), C.byref(self.h)))

    def set_state(self, x, v, p, type, rho, nu, tag=None):
        x, v, p, rho, nu, typ = _f64(x), _f64(v), _f64(p), _f64(rho), _f64(nu), _i32(type)
        dev = _on_device(x, v, p, rho, nu, typ)
        n = int(typ.numel()) if _is_torch(typ) else int(typ.size)
        _need(x, 3 * n, "x [nlocal][3]"); _need(v, 3 * n, "v [nlocal][3]"); _need(p, n, "p [nlocal]")
        _need(rho, n, "rho [nlocal]"); _need(nu, n, "nu [nlocal]")
        if self.decomp is None:
            if tag is not None:
                raise ValueError("set_state: tag belongs to the distributed driver (InsStep(ctx, params, decomp))")
            _check(lib().isph_ins_set_state(self.h, n, _ptr(x), _ptr(v), _ptr(p), _ptr(typ), _ptr(rho), _ptr(nu), dev))
            return
        if tag is None:
            raise ValueError("set_state: the distributed driver needs tag, the particles' global ids")
        tag = _i32(tag)
        _on_device(x, tag)
        _need(tag, n, "tag [nlocal]")
        args = [_ptr(a) if n else None for a in (x, v, p, typ, rho, nu, tag)]
        _check(lib().isph_ins_set_state_dist(self.h, n, *args, dev))

    def set_list(self, x_all, owner, neigh_ptr, neigh_idx):
        """the caller's ghosts (x_all [nall, 3]), owners [nall] and full list (int32 or int64 offsets [nlocal + 1])"""
        x_all, owner, nidx = _f64(x_all), _i32(owner), _i32(neigh_idx)
        wide = str(neigh_ptr.dtype) in ("int64", "torch.int64")
        nptr = (neigh_ptr if _is_torch(neigh_ptr) else np.ascontiguousarray(neigh_ptr)) if wide else _i32(neigh_ptr)
        dev = _on_device(x_all, owner, nptr, nidx)
        nall = int(owner.numel()) if _is_torch(owner) else int(owner.size)
        nl = self.sizes()["nlocal"]
        _need(x_all, 3 * nall, "x_all [nall][3]"); _need(nptr, nl + 1, "neigh_ptr [nlocal+1]")
        last = int(nptr[nl].item()) if _is_torch(nptr) else int(nptr[nl])
        _need(nidx, last, "neigh_idx [neigh_ptr[nlocal]]")
        _check(lib().isph_ins_set_list(self.h, nall, _ptr(x_all), _ptr(owner), None if wide else _ptr(nptr),
                                       _ptr(nptr) if wide else None, _ptr(nidx), dev))

    def rebuild(self):
        _check(lib().isph_ins_rebuild(self.h))

    def sizes(self):
        """dict(nlocal, nall, entries, step, pre_done, solid_present); the distributed driver adds ncol, npeers, noffrank,
        sent and received (by the last rebuild) and nglobal (the particles of all ranks)"""
        a = (C.c_longlong * 6)()
        _check(lib().isph_ins_sizes(self.h, a))
        d = dict(nlocal=int(a[0]), nall=int(a[1]), entries=int(a[2]), step=int(a[3]), pre_done=bool(a[4]),
                 solid_present=bool(a[5]))
        if self.decomp is not None:
            b = (C.c_longlong * 10)()
            _check(lib().isph_ins_sizes_dist(self.h, b))
            d.update(ncol=int(b[4]), npeers=int(b[5]), noffrank=int(b[6]), sent=int(b[7]), received=int(b[8]), nglobal=int(b[9]))
        return d

    def get(self, name, ghosts=False, device=False):
        """a copy of a field: numpy array, or a device tensor with device=True"""
        if name not in _INS_FIELDS:
            raise ValueError("unknown field %r" % name)
        per, dt = _INS_FIELDS[name]
        d = self.dim
        per = {"Gc": d * d, "Lc": d * (d + 1) // 2}.get(name, per)
        sz = self.sizes()
        rows = sz["nall"] if ghosts else sz["nlocal"]
        shape = (rows,) if per == 1 else (rows, per)
        if device:
            import torch
            out = torch.zeros(shape, dtype=torch.float64 if dt is np.float64 else torch.int32, device="cuda")
        else:
            out = np.zeros(shape, dtype=dt)
        _check(lib().isph_ins_get(self.h, name.encode(), int(ghosts), _ptr(out), int(device)))
        return out

    def pre(self):
        _check(lib().isph_ins_pre(self.h))

    def view(self):
        """the isph_particles of the state (device pointers) for the force entry points of the C ABI"""
        pv = _Particles()
        _check(lib().isph_ins_view(self.h, C.byref(pv)))
        return pv

    def force_ptr(self):
        """device address of the force [nall][3] the Helmholtz right-hand side reads (0 before pre)"""
        return int(lib().isph_ins_force(self.h) or 0)

    def add_force(self, f):
        """isph_ins_add_force: f [nlocal, 3] or [nall, 3] (numpy or device tensor) is added to the force of the step"""
        f = _f64(f)
        sz = self.sizes()
        if f.ndim != 2 or int(f.shape[1]) != 3 or int(f.shape[0]) not in (sz["nlocal"], sz["nall"]):
            raise OperandError("f: [nlocal][3] or [nall][3] needed, %s given" % (tuple(f.shape),))
        _check(lib().isph_ins_add_force(self.h, int(f.shape[0]), _ptr(f), _on_device(f)))

    def solve(self):
        info = InsInfo()
        _check(lib().isph_ins_solve(self.h, C.byref(info)))
        return info

    def advance(self):
        _check(lib().isph_ins_advance(self.h))

    def shift(self):
        vmax = C.c_double(0.0)
        _check(lib().isph_ins_shift(self.h, C.byref(vmax)))
        return vmax.value

    def diagnostics(self, t):
        out = (C.c_double * 12)()
        _check(lib().isph_ins_diagnostics(self.h, float(t), out))
        return np.array(out[:], dtype=np.float64)

    def run(self, nsteps, diag=True):
        """isph_ins_run; returns the [nsteps, 16] diagnostics (columns DIAG_FIELDS) or None"""
        out = np.zeros((int(nsteps), 16)) if diag else None
        _check(lib().isph_ins_run(self.h, int(nsteps), _ptr(out)))
        return out

    def close(self):
        if self.h:
            lib().isph_ins_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
