"""ctypes binding of libslod_hip.so (include/slod.h) for tests and bench.py.

This is plumbing only: every compute call goes through the C-ABI into the HIP kernels.
There is no CPU fallback -- loading fails loudly if the library has not been built, and
compute entry points raise SlodError if no HIP device is usable.
"""
import ctypes as C
import os
import weakref

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_PKG, "lib", "libslod_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "slod.h")


class SlodError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("slod error %d: %s" % (code, msg))
        self.code = code


class Config(C.Structure):
    _fields_ = [(k, C.c_int32) for k in (
        "dim", "spacedim", "n_global_refinements", "n_cells_per_side", "n_subdivisions",
        "oversampling", "lod_stabilization", "constant_coefficients", "projection_quirk",
        "n_problems", "device", "reserved")]


class PatchInfo(C.Structure):
    _fields_ = [("cx", C.c_int32), ("cy", C.c_int32), ("x0", C.c_int32), ("y0", C.c_int32),
                ("mx", C.c_int32), ("my", C.c_int32), ("nx", C.c_int32), ("ny", C.c_int32),
                ("side_domain", C.c_int32 * 4), ("n_fine", C.c_int32), ("n_internal", C.c_int32),
                ("n_boundary", C.c_int32), ("n_coarse", C.c_int32), ("is_lod", C.c_int32)]


class PatchDiag(C.Structure):
    """slod_patch_diag: decisions of the SLOD selection stage for one (patch, component)."""
    _fields_ = [("path", C.c_int32), ("n_cut", C.c_int32), ("n_dropped", C.c_int32), ("sweeps", C.c_int32),
                ("dinf", C.c_double), ("sigma_max", C.c_double), ("sigma_min", C.c_double)]


class ErrorNorms(C.Structure):
    """slod_error_norms: per-component L2, H1-seminorm and max-norm of e = u - v - w, and a(e,e)^{1/2}."""
    _fields_ = [("l2", C.c_double * 2), ("h1_semi", C.c_double * 2), ("linf", C.c_double * 2),
                ("energy", C.c_double), ("reserved", C.c_double * 3)]


class FactorInfo(C.Structure):
    """slod_lod_factor_info: rows, half bandwidth, tile edge, device bytes, pivot range of the banded Cholesky factor."""
    _fields_ = [("n", C.c_int32), ("half_bandwidth", C.c_int32), ("block", C.c_int32), ("bytes", C.c_uint64),
                ("min_pivot", C.c_double), ("max_pivot", C.c_double)]


class InertiaInfo(C.Structure):
    """slod_lod_factor_inertia_info: signs of D of an LDL^T factor, its pivot range in absolute value, ||S||_inf and
    || |L||D||L^T| ||_inf (their ratio is the growth)."""
    _fields_ = [("n_negative", C.c_int32), ("n_positive", C.c_int32), ("min_abs_pivot", C.c_double),
                ("max_abs_pivot", C.c_double), ("norm_matrix", C.c_double), ("norm_factor", C.c_double)]

    @property
    def growth(self):
        return self.norm_factor / self.norm_matrix


class ReceiversInfo(C.Structure):
    """slod_lod_receivers_info: receivers, members, entries of the rows per member, device bytes."""
    _fields_ = [("n_receivers", C.c_int32), ("n_members", C.c_int32), ("nnz", C.c_uint64), ("bytes", C.c_uint64)]


class TimeRecord(C.Structure):
    """slod_lod_time_record: what the next stepper call on the handle records (slod_lod_time_record_arm)."""
    _fields_ = [("recv", C.c_void_p), ("what", C.c_int), ("every", C.c_int), ("d_trace", C.c_void_p),
                ("ld_trace", C.c_size_t), ("record_stride", C.c_size_t), ("capacity", C.c_int)]


RECORD_U, RECORD_V = 1, 2   # enum slod_record_what


class SourcesInfo(C.Structure):
    """slod_lod_sources_info: sources, members, touched coarse rows, entries per member, device bytes."""
    _fields_ = [("n_sources", C.c_int32), ("n_members", C.c_int32), ("n_rows_touched", C.c_uint32), ("nnz", C.c_uint64),
                ("bytes", C.c_uint64)]


class TimeSource(C.Structure):
    """slod_lod_time_source: what drives the next stepper call on the handle (slod_lod_time_source_arm)."""
    _fields_ = [("src", C.c_void_p), ("d_signal", C.c_void_p), ("ld_signal", C.c_size_t), ("sample_stride", C.c_size_t),
                ("n_samples", C.c_int)]


_lib = None


def load():
    """Load libslod_hip.so; raises OSError if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    # tools/ may point at the timing-experiment build (lib/libslod_hip_diag.so, `make diag`)
    path = os.environ.get("SLOD_LIB_PATH", LIB_PATH)
    if not os.path.exists(path):
        raise OSError("%s not built: run `make -C dealii-slod_amd` "
                      "(or __graft_entry__.build()); there is no CPU fallback" % path)
    # One HIP runtime per process: PyTorch ships its own libamdhip64 (soname libamdhip64.so.7,
    # the same as /opt/rocm's).  If torch is imported AFTER this library, a second runtime
    # gets loaded and whichever initialises second sees no device.  Importing torch first
    # makes libslod_hip bind to torch's copy (torch is only plumbing here: device memory,
    # streams, torch.distributed).  Non-Python users link /opt/rocm's runtime as usual.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    vp, dp, u32p, u64p = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    lib.slod_abi_version.restype = C.c_int
    lib.slod_last_error.restype = C.c_char_p
    lib.slod_last_error.argtypes = [vp]
    lib.slod_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    lib.slod_destroy.argtypes = [vp]
    lib.slod_destroy.restype = None
    lib.slod_num_patches.argtypes = [vp]
    lib.slod_patch_layout.argtypes = [vp, C.c_uint32, C.POINTER(PatchInfo)]
    lib.slod_patch_cells.argtypes = [vp, C.c_uint32, u32p, C.c_size_t]
    lib.slod_patch_dof_permutation.argtypes = [vp, C.c_uint32, u32p, C.c_size_t]
    lib.slod_partition.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, u64p, u64p]
    lib.slod_set_coefficient.argtypes = [vp, C.c_uint32, C.c_int, vp, C.c_int, C.c_size_t, C.c_int]
    lib.slod_plan_create.argtypes = [vp, u32p, C.c_size_t, u64p, C.POINTER(vp)]
    lib.slod_plan_destroy.argtypes = [vp]
    lib.slod_plan_destroy.restype = None
    lib.slod_plan_stride.argtypes = [vp]
    lib.slod_plan_stride.restype = C.c_size_t
    lib.slod_plan_output_size.argtypes = [vp]
    lib.slod_plan_output_size.restype = C.c_size_t
    lib.slod_plan_execute.argtypes = [vp, vp, vp, vp]
    lib.slod_plan_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.slod_plan_profile.argtypes = [vp, C.c_int]
    lib.slod_plan_status.argtypes = [vp]
    lib.slod_plan_patch_layout.argtypes = [vp, C.c_size_t, C.c_int, C.POINTER(PatchInfo), u32p]
    lib.slod_plan_set_overlap.argtypes = [vp, C.c_int]
    lib.slod_plan_join.argtypes = [vp, vp]
    lib.slod_plan_diagnostics.argtypes = [vp, C.POINTER(PatchDiag), C.c_size_t]
    lib.slod_compute_basis.argtypes = [vp, u32p, C.c_size_t, dp, dp, u64p]
    lib.slod_comm_last_error.restype = C.c_char_p
    lib.slod_comm_last_error.argtypes = [vp]
    lib.slod_comm_unique_id.argtypes = [C.c_char_p]
    lib.slod_comm_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    lib.slod_comm_destroy.argtypes = [vp]
    lib.slod_comm_destroy.restype = None
    lib.slod_comm_allgather.argtypes = [vp, vp, vp, C.c_size_t, vp]
    lib.slod_gather_piece.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, u64p, u64p]
    lib.slod_plan_execute_allgather.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_int, vp, vp]
    lib.slod_lod_row_capacity.argtypes = [vp]
    lib.slod_lod_pattern.argtypes = [vp, C.c_uint32, u32p, C.c_size_t]
    lib.slod_lod_matrix.argtypes = [vp, u32p, C.c_size_t, vp, vp, C.c_size_t, vp, vp, vp]
    lib.slod_lod_rhs.argtypes = [vp, u32p, C.c_size_t, vp, C.c_size_t, vp, vp, vp]
    lib.slod_lod_solve.argtypes = [vp, vp, vp, vp, vp, C.c_double, C.c_int, dp]
    lib.slod_lod_reconstruct.argtypes = [vp, vp, C.c_size_t, vp, vp, vp]
    lib.slod_lod_rhs_multi.argtypes = [vp, u32p, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.c_int, vp, C.c_size_t, vp]
    lib.slod_lod_solve_multi.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_int, vp, C.c_size_t, C.c_double, C.c_int,
                                         C.POINTER(C.c_int), dp]
    lib.slod_lod_reconstruct_multi.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int, vp, C.c_size_t, vp]
    lib.slod_lod_mass_matrix.argtypes = [vp, u32p, C.c_size_t, vp, C.c_size_t, vp, vp, vp, vp]
    lib.slod_lod_apply_multi.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_int, vp, C.c_size_t, vp]
    lib.slod_lod_matrix_combine.argtypes = [vp, C.c_double, vp, C.c_double, vp, vp, vp]
    lib.slod_lod_theta_steps.argtypes = [vp, vp, vp, vp, C.c_double, C.c_double, C.c_int, C.c_int, vp, C.c_size_t, vp,
                                         C.c_size_t, C.c_size_t, C.c_double, C.c_int, C.POINTER(C.c_int), dp]
    lib.slod_lod_matrix_symmetrize.argtypes = [vp, vp, vp, vp, vp]
    lib.slod_lod_eigs.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, C.c_double, C.c_int, C.c_double,
                                  C.c_int, dp, dp, C.POINTER(C.c_int)]
    lib.slod_lod_inner_multi.argtypes = [vp, vp, vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int, dp, vp]
    lib.slod_lod_newmark_accel.argtypes = [vp, vp, vp, vp, C.c_double, C.c_double, C.c_int, vp, C.c_size_t, vp, C.c_size_t,
                                           vp, C.c_size_t, vp, C.c_size_t, C.c_double, C.c_int, C.POINTER(C.c_int), dp]
    lib.slod_lod_newmark_steps.argtypes = [vp, vp, vp, vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                           C.c_int, C.c_int, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t,
                                           C.c_size_t, C.c_double, C.c_int, C.POINTER(C.c_int), dp, dp, dp]
    lib.slod_lod_factor_create.argtypes = [vp, vp, vp, C.POINTER(vp)]
    lib.slod_lod_factor_get_info.argtypes = [vp, C.POINTER(FactorInfo)]
    lib.slod_lod_factor_solve.argtypes = [vp, vp, C.c_size_t, C.c_int, vp, C.c_size_t, vp]
    lib.slod_lod_factor_destroy.argtypes = [vp]
    lib.slod_lod_factor_destroy.restype = None
    lib.slod_lod_theta_steps_direct.argtypes = [vp, vp, vp, vp, C.c_double, C.c_double, C.c_int, C.c_int, vp, C.c_size_t, vp,
                                                C.c_size_t, C.c_size_t]
    lib.slod_lod_newmark_accel_direct.argtypes = [vp, vp, vp, vp, vp, C.c_double, C.c_double, C.c_int, vp, C.c_size_t, vp,
                                                  C.c_size_t, vp, C.c_size_t, vp, C.c_size_t]
    lib.slod_lod_newmark_steps_direct.argtypes = [vp, vp, vp, vp, vp, C.c_double, C.c_double, C.c_double, C.c_double,
                                                  C.c_double, C.c_int, C.c_int, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t,
                                                  vp, C.c_size_t, C.c_size_t, dp, dp]
    lib.slod_lod_matrix_ensemble.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_int, vp, C.c_size_t, vp, vp]
    lib.slod_lod_rhs_ensemble.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, vp, C.c_size_t, vp, C.c_size_t, vp]
    lib.slod_lod_apply_ensemble.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_size_t, C.c_int, vp, C.c_size_t, vp]
    lib.slod_lod_solve_ensemble.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_size_t, C.c_int, vp, C.c_size_t, C.c_double,
                                            C.c_int, C.POINTER(C.c_int), dp]
    lib.slod_lod_reconstruct_ensemble.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, vp, C.c_size_t, vp, C.c_size_t, vp]
    lib.slod_ensemble_moments.argtypes = [vp, vp, C.c_size_t, C.c_int, C.c_size_t, vp, vp, vp]
    lib.slod_lod_mass_matrix_ensemble.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, vp, C.c_size_t, vp, C.c_size_t, vp, vp]
    lib.slod_lod_matrix_symmetrize_ensemble.argtypes = [vp, vp, C.c_size_t, vp, C.c_int, vp, C.c_size_t, vp]
    lib.slod_lod_matrix_combine_ensemble.argtypes = [vp, C.c_double, vp, C.c_size_t, C.c_double, vp, C.c_size_t, C.c_int, vp,
                                                     C.c_size_t, vp]
    lib.slod_lod_factor_create_ensemble.argtypes = [vp, vp, C.c_size_t, C.c_int, vp, C.POINTER(C.c_int32), C.POINTER(vp)]
    lib.slod_lod_factor_get_info_member.argtypes = [vp, C.c_int, C.POINTER(FactorInfo)]
    lib.slod_lod_factor_solve_ensemble.argtypes = [vp, C.c_int, C.c_int, vp, C.c_size_t, C.c_int, vp, C.c_size_t, vp]
    lib.slod_lod_solve_multi_precond.argtypes = [vp, vp, vp, vp, vp, C.c_size_t, C.c_int, vp, C.c_size_t, C.c_double, C.c_int,
                                                 C.POINTER(C.c_int), dp]
    lib.slod_lod_solve_ensemble_precond.argtypes = [vp, vp, vp, C.c_size_t, vp, vp, C.c_size_t, C.c_int, vp, C.c_size_t,
                                                    C.c_double, C.c_int, C.POINTER(C.c_int), dp]
    lib.slod_lod_theta_steps_ensemble_direct.argtypes = [vp, vp, vp, C.c_size_t, vp, C.c_double, C.c_double, C.c_int, C.c_int, vp,
                                                         C.c_size_t, vp, C.c_size_t, C.c_size_t]
    lib.slod_lod_inner_ensemble.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int, dp, vp]
    lib.slod_lod_newmark_accel_ensemble_direct.argtypes = [vp, vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_double, C.c_double,
                                                           C.c_int, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t]
    lib.slod_lod_newmark_steps_ensemble_direct.argtypes = [vp, vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_double, C.c_double,
                                                           C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, vp, C.c_size_t,
                                                           vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, dp, dp]
    lib.slod_lod_eigs_direct.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, C.c_double, C.c_int, dp, dp]
    lib.slod_lod_eigs_ensemble_direct.argtypes = [vp, vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                                  vp, C.c_size_t, C.c_double, C.c_int, dp, dp, C.POINTER(C.c_int)]
    lib.slod_lod_factor_create_ldl.argtypes = [vp, vp, vp, C.POINTER(vp)]
    lib.slod_lod_factor_create_ldl_ensemble.argtypes = [vp, vp, C.c_size_t, C.c_int, vp, C.POINTER(C.c_int32), C.POINTER(vp)]
    lib.slod_lod_factor_inertia.argtypes = [vp, C.c_int, C.POINTER(InertiaInfo)]
    lib.slod_lod_eigs_shift_direct.argtypes = [vp, vp, C.c_double, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t,
                                               C.c_double, C.c_int, dp, dp]
    lib.slod_lod_eigs_shift_ensemble_direct.argtypes = [vp, vp, C.c_double, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_int, C.c_int,
                                                        C.c_int, C.c_int, vp, C.c_size_t, C.c_double, C.c_int, dp, dp,
                                                        C.POINTER(C.c_int)]
    lib.slod_lod_factor_create_zldl.argtypes = [vp, vp, vp, vp, dp, dp, C.c_int, C.POINTER(C.c_int32), C.POINTER(vp)]
    lib.slod_lod_factor_solve_complex.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_size_t, C.c_int, C.c_int, vp, vp, C.c_size_t, vp]
    lib.slod_lod_harmonic_response.argtypes = [vp, vp, vp, vp, C.c_double, C.c_double, dp, C.c_int, vp, vp, C.c_size_t, C.c_int,
                                               vp, vp, C.c_size_t, dp, dp]
    lib.slod_lod_factor_create_zldl_ensemble.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_int, vp, dp, dp, C.c_int,
                                                         C.POINTER(C.c_int32), C.POINTER(vp)]
    lib.slod_lod_factor_solve_complex_ensemble.argtypes = [vp, C.c_int, C.c_int, vp, vp, C.c_size_t, C.c_int, C.c_int, vp, vp,
                                                           C.c_size_t, vp]
    lib.slod_lod_harmonic_response_ensemble.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_int, C.c_double, C.c_double, dp,
                                                        C.c_int, vp, vp, C.c_size_t, C.c_int, vp, vp, C.c_size_t, dp, dp, dp]
    lib.slod_lod_irk_coefficients.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, dp, dp]
    lib.slod_lod_irk_heat_steps_direct.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, C.c_double, C.c_int, C.c_int, vp, C.c_size_t,
                                                   vp, C.c_size_t, C.c_size_t]
    lib.slod_lod_irk_wave_steps_direct.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_double, C.c_double, C.c_double,
                                                   C.c_int, C.c_int, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t,
                                                   dp, dp]
    lib.slod_lod_irk_heat_steps_ensemble_direct.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp, C.c_double, C.c_int,
                                                            C.c_int, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t]
    lib.slod_lod_irk_wave_steps_ensemble_direct.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp, C.c_size_t, vp,
                                                            C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, vp, C.c_size_t,
                                                            vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, dp, dp]
    lib.slod_lod_newmark_accel_damped.argtypes = [vp, vp, vp, vp, vp, C.c_double, C.c_double, C.c_int, vp, C.c_size_t, vp,
                                                  C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, C.c_double, C.c_int,
                                                  C.POINTER(C.c_int), dp]
    lib.slod_lod_newmark_steps_damped.argtypes = [vp, vp, vp, vp, vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                                  C.c_int, C.c_int, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, vp,
                                                  C.c_size_t, C.c_size_t, C.c_double, C.c_int, C.POINTER(C.c_int), dp, dp, dp]
    lib.slod_lod_newmark_accel_damped_direct.argtypes = [vp, vp, vp, vp, vp, vp, C.c_double, C.c_double, C.c_int, vp, C.c_size_t,
                                                         vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t]
    lib.slod_lod_newmark_steps_damped_direct.argtypes = [vp, vp, vp, vp, vp, vp, C.c_double, C.c_double, C.c_double, C.c_double,
                                                         C.c_double, C.c_int, C.c_int, vp, C.c_size_t, vp, C.c_size_t, vp,
                                                         C.c_size_t, vp, C.c_size_t, C.c_size_t, dp, dp]
    lib.slod_lod_factor_create_zldl3.argtypes = [vp, vp, vp, vp, vp, dp, dp, dp, C.c_int, C.POINTER(C.c_int32), C.POINTER(vp)]
    lib.slod_lod_irk_damping_coefficient.argtypes = [C.c_int, C.c_double, dp]
    lib.slod_lod_irk_wave_steps_damped_direct.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, C.c_double, C.c_double,
                                                          C.c_double, C.c_int, C.c_int, vp, C.c_size_t, vp, C.c_size_t, vp,
                                                          C.c_size_t, C.c_size_t, dp, dp]
    lib.slod_lod_harmonic_response_damped.argtypes = [vp, vp, vp, vp, vp, C.c_double, C.c_double, dp, C.c_int, vp, vp, C.c_size_t,
                                                      C.c_int, vp, vp, C.c_size_t, dp, dp, dp]
    lib.slod_lod_receiver_capacity.argtypes = [vp]
    lib.slod_lod_receiver_pattern.argtypes = [vp, C.c_uint32, u32p, C.c_size_t]
    lib.slod_lod_receivers_create.argtypes = [vp, C.c_int, u32p, u32p, C.POINTER(C.c_int32), dp, vp, C.c_size_t, C.c_size_t,
                                              C.c_int, C.POINTER(vp)]
    lib.slod_lod_receivers_get_info.argtypes = [vp, C.POINTER(ReceiversInfo)]
    lib.slod_lod_receivers_rows.argtypes = [vp, C.c_int, u32p, u32p, dp]
    lib.slod_lod_receivers_destroy.argtypes = [vp]
    lib.slod_lod_receivers_destroy.restype = None
    lib.slod_lod_observe_multi.argtypes = [vp, vp, vp, C.c_size_t, C.c_int, vp, C.c_size_t, vp]
    lib.slod_lod_observe_ensemble.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp, C.c_size_t, vp]
    lib.slod_lod_time_record_arm.argtypes = [vp, C.POINTER(TimeRecord)]
    lib.slod_lod_sources_create.argtypes = [vp, vp, C.POINTER(vp)]
    lib.slod_lod_sources_get_info.argtypes = [vp, C.POINTER(SourcesInfo)]
    lib.slod_lod_sources_destroy.argtypes = [vp]
    lib.slod_lod_sources_destroy.restype = None
    lib.slod_lod_inject_multi.argtypes = [vp, vp, vp, C.c_size_t, C.c_int, vp, C.c_size_t, vp, C.c_size_t, vp]
    lib.slod_lod_inject_ensemble.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, vp]
    lib.slod_lod_time_source_arm.argtypes = [vp, C.POINTER(TimeSource)]
    lib.slod_update_coefficient.argtypes = [vp, C.c_uint32, C.c_int, vp, C.c_int, C.c_size_t, C.c_int, vp]
    lib.slod_dirty_patches.argtypes = [vp, vp, u32p, C.c_size_t]
    lib.slod_plan_create_dirty.argtypes = [vp, C.c_uint32, vp, C.POINTER(vp)]
    lib.slod_lod_matrix_update.argtypes = [vp, vp, vp, vp, C.c_size_t, vp, C.c_size_t, vp]
    lib.slod_lod_mass_matrix_update.argtypes = [vp, vp, vp, C.c_size_t, vp, vp, vp]
    lib.slod_fem_rhs.argtypes = [vp, vp, vp, vp]
    lib.slod_fem_solve.argtypes = [vp, C.c_uint32, vp, vp, C.c_double, C.c_int, dp]
    lib.slod_coarse_coefficient.argtypes = [vp, C.c_uint32, C.c_int, vp, vp]
    lib.slod_coarse_fem_rhs.argtypes = [vp, vp, vp, vp]
    lib.slod_coarse_fem_solve.argtypes = [vp, C.c_uint32, vp, vp, C.c_double, C.c_int, dp]
    lib.slod_coarse_interpolate.argtypes = [vp, vp, vp, vp]
    lib.slod_compute_error_norms.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, C.POINTER(ErrorNorms), vp]
    lib.slod_device_patch_layout.argtypes = [vp, u32p, C.c_size_t, C.POINTER(PatchInfo)]
    lib.slod_sample_coefficient.argtypes = [vp, C.c_uint32, C.c_int, vp, C.c_int]
    lib.slod_assemble_stiffness_for_patch.argtypes = [vp, C.c_uint32, dp]
    lib.slod_patch_solution.argtypes = [vp, C.c_uint32, dp]
    _lib = lib
    return lib


def declared_symbols():
    """Entry points declared in include/slod.h (used by the symbol-export test)."""
    import re
    txt = open(HEADER_PATH).read()
    return sorted(set(re.findall(r"\b(slod_[a-z_0-9]+)\s*\(", txt)))


def partition(n_total, n_ranks, rank):
    b, e = C.c_uint64(), C.c_uint64()
    rc = load().slod_partition(n_total, n_ranks, rank, C.byref(b), C.byref(e))
    if rc:
        raise SlodError(rc, "slod_partition: bad arguments")
    return b.value, e.value


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def gather_piece(patches_per_rank, n_pieces, piece):
    f, c = C.c_uint64(), C.c_uint64()
    rc = load().slod_gather_piece(patches_per_rank, n_pieces, piece, C.byref(f), C.byref(c))
    if rc:
        raise SlodError(rc, "slod_gather_piece: bad arguments")
    return f.value, c.value


class Comm:
    """slod_comm: RCCL communicator of the C-ABI (what a C++ host uses; bench.py's N > 1 path goes
    through torch.distributed instead)."""

    def __init__(self, comm_id, n_ranks, rank, device=0):
        self.lib = load()
        self.c = C.c_void_p()
        rc = self.lib.slod_comm_create(comm_id, n_ranks, rank, device, C.byref(self.c))
        if rc:
            raise SlodError(rc, self.lib.slod_comm_last_error(None).decode())
        self.n_ranks, self.rank = n_ranks, rank

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        rc = load().slod_comm_unique_id(buf)
        if rc:
            raise SlodError(rc, load().slod_comm_last_error(None).decode())
        return buf.raw

    def allgather(self, d_send, d_recv, count, stream):
        rc = self.lib.slod_comm_allgather(self.c, d_send, d_recv, count, stream)
        if rc:
            raise SlodError(rc, self.lib.slod_comm_last_error(self.c).decode())

    def close(self):
        if self.c:
            self.lib.slod_comm_destroy(self.c)
            self.c = None


class Plan:
    def __init__(self, slod, gids, offsets=None, dirty=None):
        """dirty = (problem, d_dirty): the plan of slod_plan_create_dirty; gids are then read from the dirty array."""
        self.slod = slod
        self.lib = slod.lib
        if dirty is not None:
            problem, d_dirty = dirty
            self.p = C.c_void_p()
            n = self.lib.slod_plan_create_dirty(slod.h, problem, d_dirty, C.byref(self.p))
            if n < 0:
                slod._check(n)
            ids = np.zeros(max(n, 1), dtype=np.uint32)
            m = self.lib.slod_dirty_patches(slod.h, d_dirty, ids.ctypes.data_as(C.POINTER(C.c_uint32)), n)
            assert m == n, "the dirty array changed under the plan"
            self.gids = ids[:n] + np.uint32(problem * slod.num_patches)
            self.stride = self.lib.slod_plan_stride(self.p)
            self.offsets = (self.gids % np.uint32(slod.num_patches)).astype(np.uint64) * np.uint64(self.stride)
            self.output_size = self.lib.slod_plan_output_size(self.p)
            return
        self.gids = np.ascontiguousarray(gids, dtype=np.uint32)
        off_p = None
        if offsets is not None:
            self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            off_p = self.offsets.ctypes.data_as(C.POINTER(C.c_uint64))
        self.p = C.c_void_p()
        rc = self.lib.slod_plan_create(slod.h, self.gids.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       len(self.gids), off_p, C.byref(self.p))
        slod._check(rc)
        self.stride = self.lib.slod_plan_stride(self.p)
        self.output_size = self.lib.slod_plan_output_size(self.p)

    def execute(self, d_basis_ptr, d_premult_ptr, stream_ptr=None):
        """Asynchronous launch; arguments are raw device pointers (ints)."""
        self.slod._check(self.lib.slod_plan_execute(self.p, d_basis_ptr, d_premult_ptr, stream_ptr))

    def execute_allgather(self, comm, d_basis_all, d_premult_all, patches_per_rank, n_pieces, compute_stream,
                          comm_stream):
        self.slod._check(self.lib.slod_plan_execute_allgather(self.p, comm.c, d_basis_all, d_premult_all,
                                                              patches_per_rank, n_pieces, compute_stream, comm_stream))

    def profile(self, depth):
        self.slod._check(self.lib.slod_plan_profile(self.p, depth))

    def kernel_ms(self):
        ms = (C.c_float * 3)()
        self.slod._check(self.lib.slod_plan_kernel_ms(self.p, ms))
        return [float(x) for x in ms]

    def status(self):
        self.slod._check(self.lib.slod_plan_status(self.p))

    def set_overlap(self, depth):
        """depth 2: consecutive executes overlap on two internal streams (join() / status() order the caller after them)."""
        self.slod._check(self.lib.slod_plan_set_overlap(self.p, depth))

    def join(self, stream_ptr=None):
        self.slod._check(self.lib.slod_plan_join(self.p, stream_ptr))

    def patch_layout(self, k, launch_order=False):
        """(PatchInfo, plan_index) of the k-th descriptor the kernels launch with (device read-back)."""
        info, idx = PatchInfo(), C.c_uint32()
        self.slod._check(self.lib.slod_plan_patch_layout(self.p, k, 1 if launch_order else 0, C.byref(info), C.byref(idx)))
        return info, idx.value

    def diagnostics(self):
        """[(patch k, component d)] -> PatchDiag of the last execute."""
        n = len(self.gids) * self.slod.spacedim
        buf = (PatchDiag * max(n, 1))()
        rc = self.lib.slod_plan_diagnostics(self.p, buf, n)
        if rc < 0:
            self.slod._check(rc)
        return [buf[i] for i in range(n)]

    def close(self):
        if self.p:
            self.lib.slod_plan_destroy(self.p)
            self.p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Factor:
    """slod_lod_factor: the banded Cholesky factor of a full set of block rows; factor once, solve many.  ldl=True: the
    banded LDL^T factor of a symmetric, possibly indefinite matrix (slod_lod_factor_create_ldl), with .inertia()."""

    def __init__(self, slod, d_values, d_cols, ldl=False):
        self.slod, self.lib = slod, slod.lib
        self.f = C.c_void_p()
        create = self.lib.slod_lod_factor_create_ldl if ldl else self.lib.slod_lod_factor_create
        slod._check(create(slod.h, d_values, d_cols, C.byref(self.f)))
        self.info = FactorInfo()
        slod._check(self.lib.slod_lod_factor_get_info(self.f, C.byref(self.info)))
        slod._factors.add(self)                        # the handle closes its factors before itself

    def solve(self, d_rhs, d_u, n_rhs=1, ld_rhs=None, ld_u=None, stream=None):
        """U = A^-1 RHS on coarse multi-vectors (ld defaults to n_rhs); d_u may be d_rhs.  Asynchronous."""
        self.slod._check(self.lib.slod_lod_factor_solve(self.f, d_rhs, n_rhs if ld_rhs is None else ld_rhs, n_rhs, d_u,
                                                        n_rhs if ld_u is None else ld_u, stream))

    def inertia(self, member=0):
        """slod_lod_factor_inertia of an LDL^T factor: InertiaInfo (n_negative, n_positive, min_abs_pivot, max_abs_pivot,
        norm_matrix, norm_factor, .growth).  SlodError(-1) on a Cholesky factor."""
        info = InertiaInfo()
        self.slod._check(self.lib.slod_lod_factor_inertia(self.f, member, C.byref(info)))
        return info

    def close(self):
        if self.f:
            self.lib.slod_lod_factor_destroy(self.f)
            self.f = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EnsembleFactor(Factor):
    """slod_lod_factor of an ensemble matrix: a factor per member in one object.  .info is the range over all members,
    .member_info(k) that of member k, .bad_pivot the first non-positive pivot per member (-1 everywhere on success).
    When a member fails, SlodError(-5) carries .bad_pivot; drop those members and factor again."""

    def __init__(self, slod, d_values, d_cols, n_members, ld_m=None, ldl=False):
        self.slod, self.lib, self.n_members = slod, slod.lib, n_members
        self.f = C.c_void_p()
        self.bad_pivot = np.full(max(n_members, 1), -1, dtype=np.int32)
        create = self.lib.slod_lod_factor_create_ldl_ensemble if ldl else self.lib.slod_lod_factor_create_ensemble
        rc = create(slod.h, d_values, n_members if ld_m is None else ld_m, n_members, d_cols,
                    self.bad_pivot.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(self.f))
        if rc:
            err = SlodError(rc, self.lib.slod_last_error(slod.h).decode())
            err.bad_pivot = self.bad_pivot[:max(n_members, 0)].copy()
            raise err
        self.info = FactorInfo()
        slod._check(self.lib.slod_lod_factor_get_info(self.f, C.byref(self.info)))
        slod._factors.add(self)

    def member_info(self, member):
        info = FactorInfo()
        self.slod._check(self.lib.slod_lod_factor_get_info_member(self.f, member, C.byref(info)))
        return info

    def solve(self, d_rhs, d_u, n_rhs=1, first_member=0, n_members=None, ld_rhs=None, ld_u=None, stream=None):
        """Member first_member + k solves the columns k * n_rhs .. of d_rhs into d_u (ld defaults to n_members * n_rhs);
        d_u may be d_rhs.  Asynchronous."""
        K = self.n_members - first_member if n_members is None else n_members
        self.slod._check(self.lib.slod_lod_factor_solve_ensemble(self.f, first_member, K, d_rhs, K * n_rhs if ld_rhs is None else ld_rhs,
                                                                 n_rhs, d_u, K * n_rhs if ld_u is None else ld_u, stream))


class ComplexFactor(EnsembleFactor):
    """slod_lod_factor of slod_lod_factor_create_zldl: the complex symmetric S_k = alpha_k A + beta_k B = L D L^T of every
    member k in one object.  alpha, beta: complex scalars or sequences of n_members.  .info / .member_info(k) give the
    range of |D|, .inertia(k) the two norms (n_negative = n_positive = -1), .bad_pivot as EnsembleFactor.
    matrix_members = K (slod_lod_factor_create_zldl_ensemble): d_a, d_b are ensemble matrices of K members, alpha and beta
    have one entry per coefficient pair, and the factor member j = k K + m is pair k on the matrices of member m
    (.n_members = len(alpha) * K, .n_coef = len(alpha)).
    d_c, gamma (slod_lod_factor_create_zldl3, single matrices only): S_k = alpha_k A + beta_k B + gamma_k C."""

    def __init__(self, slod, d_a, d_b, d_cols, alpha, beta, matrix_members=None, ld_a_m=None, ld_b_m=None, d_c=None,
                 gamma=None):
        self.slod, self.lib = slod, slod.lib
        self.alpha = np.atleast_1d(np.asarray(alpha, dtype=np.complex128)).copy()
        self.beta = np.atleast_1d(np.asarray(beta, dtype=np.complex128)).copy()
        if self.alpha.shape != self.beta.shape or self.alpha.ndim != 1:
            raise ValueError("alpha and beta: one complex number per member each")
        self.n_coef = len(self.alpha)
        self.matrix_members = matrix_members
        self.n_members = n_members = self.n_coef * (1 if matrix_members is None else max(matrix_members, 0))
        self.f = C.c_void_p()
        self.bad_pivot = np.full(max(n_members, 1), -1, dtype=np.int32)
        if gamma is not None:
            if matrix_members is not None:
                raise ValueError("a third term takes single matrices")
            self.gamma = np.atleast_1d(np.asarray(gamma, dtype=np.complex128)).copy()
            if self.gamma.shape != self.alpha.shape:
                raise ValueError("gamma: one complex number per member")
            rc = self.lib.slod_lod_factor_create_zldl3(slod.h, d_a, d_b, d_c, d_cols, _dp(self.alpha.view(np.float64)),
                                                       _dp(self.beta.view(np.float64)), _dp(self.gamma.view(np.float64)),
                                                       n_members, self.bad_pivot.ctypes.data_as(C.POINTER(C.c_int32)),
                                                       C.byref(self.f))
        elif matrix_members is None:
            rc = self.lib.slod_lod_factor_create_zldl(slod.h, d_a, d_b, d_cols, _dp(self.alpha.view(np.float64)),
                                                      _dp(self.beta.view(np.float64)), n_members,
                                                      self.bad_pivot.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(self.f))
        else:
            K = matrix_members
            rc = self.lib.slod_lod_factor_create_zldl_ensemble(
                slod.h, d_a, K if ld_a_m is None else ld_a_m, d_b, K if ld_b_m is None else ld_b_m, K, d_cols,
                _dp(self.alpha.view(np.float64)), _dp(self.beta.view(np.float64)), self.n_coef,
                self.bad_pivot.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(self.f))
        if rc:
            err = SlodError(rc, self.lib.slod_last_error(slod.h).decode())
            err.bad_pivot = self.bad_pivot[:n_members].copy()
            raise err
        self.info = FactorInfo()
        slod._check(self.lib.slod_lod_factor_get_info(self.f, C.byref(self.info)))
        slod._factors.add(self)

    def solve_complex(self, d_rhs_re, d_rhs_im, d_u_re, d_u_im, n_rhs=1, first_member=0, n_members=None, shared_rhs=False,
                      ld_rhs=None, ld_u=None, stream=None, rhs_members=None):
        """Member first_member + k solves the columns k * n_rhs .. of (d_rhs_re, d_rhs_im) into (d_u_re, d_u_im);
        shared_rhs: every member reads the columns 0 .. n_rhs - 1.  d_rhs_im None: a real rhs.  ld defaults to
        n_members * n_rhs (the shared rhs: n_rhs).  Asynchronous.
        rhs_members=R (slod_lod_factor_solve_complex_ensemble): factor member j reads the rhs columns (j % R) * n_rhs ..
        and writes the columns (j - first_member) * n_rhs ..; ld_rhs defaults to R * n_rhs."""
        K = self.n_members - first_member if n_members is None else n_members
        if rhs_members is not None:
            if shared_rhs:
                raise ValueError("shared_rhs is rhs_members=1")
            self.slod._check(self.lib.slod_lod_factor_solve_complex_ensemble(
                self.f, first_member, K, d_rhs_re, d_rhs_im, max(rhs_members, 1) * n_rhs if ld_rhs is None else ld_rhs, n_rhs,
                rhs_members, d_u_re, d_u_im, K * n_rhs if ld_u is None else ld_u, stream))
            return
        if ld_rhs is None:
            ld_rhs = n_rhs if shared_rhs else K * n_rhs
        self.slod._check(self.lib.slod_lod_factor_solve_complex(self.f, first_member, K, d_rhs_re, d_rhs_im, ld_rhs, n_rhs,
                                                                1 if shared_rhs else 0, d_u_re, d_u_im,
                                                                K * n_rhs if ld_u is None else ld_u, stream))


def sponge_profile(NE, width, sigma_max):
    """The damping coefficient of a sponge layer per fine element, [NE * NE] with ex fastest (the d_rho of lod_mass_matrix):
    sigma = sigma_max * max(0, 1 - d / width)^2, d the distance of the element's centre from the rim of the unit square."""
    if not (NE >= 1 and width > 0.0 and sigma_max >= 0.0):
        raise ValueError("sponge_profile: NE >= 1, width > 0, sigma_max >= 0")
    x = (np.arange(NE) + 0.5) / NE
    d1 = np.minimum(x, 1.0 - x)
    d = np.minimum(d1[:, None], d1[None, :])                      # [ey][ex]
    return np.ascontiguousarray((sigma_max * np.maximum(0.0, 1.0 - d / width) ** 2).reshape(-1), dtype=np.float64)


def point_terms(NE, s, x, y, comp=0):
    """The four bilinear terms [(node, comp, weight)] of component comp of the FE function at the point (x, y) of the unit
    square on the fine grid of NE x NE elements: nodes (ex, ey), (ex+1, ey), (ex, ey+1), (ex+1, ey+1) of the element that
    holds the point.  The weights sum to 1; for a point on a node they are (1, 0, 0, 0).  Host only."""
    if not (0.0 <= x <= 1.0 and 0.0 <= y <= 1.0) or not 0 <= comp < s:
        raise ValueError("point_terms: a point of the unit square and a component below s")
    fx, fy = x * NE, y * NE
    ex, ey = min(int(np.floor(fx)), NE), min(int(np.floor(fy)), NE)
    tx, ty = fx - ex, fy - ey
    x1, y1 = min(ex + 1, NE), min(ey + 1, NE)          # on the far boundary the weight of the missing node is 0
    NEp = NE + 1
    return [(ex + ey * NEp, comp, (1.0 - tx) * (1.0 - ty)), (x1 + ey * NEp, comp, tx * (1.0 - ty)),
            (ex + y1 * NEp, comp, (1.0 - tx) * ty), (x1 + y1 * NEp, comp, tx * ty)]


class Receivers:
    """slod_lod_receivers: the rows O = W C of a set of receivers over the coarse unknowns, built from the basis slab.
    receivers: a sequence of receivers, each a sequence of terms (node, comp, weight); or term_begin/term_node/term_comp/
    term_weight arrays as the C call takes them (raw=True).  .info (n_receivers, n_members, nnz, bytes), .rows(member),
    .observe(...), .observe_ensemble(...), .close()."""

    def __init__(self, slod, receivers, d_basis, stride, n_members=1, member_stride=None, raw=False):
        self.slod, self.lib = slod, slod.lib
        self.r = C.c_void_p()
        if raw:
            begin, node, comp, weight = receivers
            n_recv = len(begin) - 1
        else:
            n_recv = len(receivers)
            begin = np.concatenate([[0], np.cumsum([len(t) for t in receivers])]) if n_recv else np.zeros(1)
            flat = [t for r in receivers for t in r]
            node, comp, weight = [t[0] for t in flat], [t[1] for t in flat], [t[2] for t in flat]
        self.term_begin = np.ascontiguousarray(begin, dtype=np.uint32)
        self.term_node = np.ascontiguousarray(node, dtype=np.uint32)
        self.term_comp = np.ascontiguousarray(comp, dtype=np.int32)
        self.term_weight = np.ascontiguousarray(weight, dtype=np.float64)
        u32p = C.POINTER(C.c_uint32)
        slod._check(self.lib.slod_lod_receivers_create(
            slod.h, n_recv, self.term_begin.ctypes.data_as(u32p), self.term_node.ctypes.data_as(u32p),
            self.term_comp.ctypes.data_as(C.POINTER(C.c_int32)), _dp(self.term_weight), d_basis, stride,
            slod.num_patches * stride if member_stride is None else member_stride, n_members, C.byref(self.r)))
        self.info = ReceiversInfo()
        slod._check(self.lib.slod_lod_receivers_get_info(self.r, C.byref(self.info)))
        self.n_recv, self.n_members = self.info.n_receivers, self.info.n_members
        slod._factors.add(self)                        # the handle closes its objects before itself

    def rows(self, member=0):
        """(row_begin[n_recv + 1], cols[nnz], values[nnz]) of one member, host arrays.  Synchronises."""
        rb = np.zeros(self.n_recv + 1, dtype=np.uint32)
        cols = np.zeros(max(self.info.nnz, 1), dtype=np.uint32)
        vals = np.zeros(max(self.info.nnz, 1))
        u32p = C.POINTER(C.c_uint32)
        self.slod._check(self.lib.slod_lod_receivers_rows(self.r, member, rb.ctypes.data_as(u32p), cols.ctypes.data_as(u32p),
                                                          _dp(vals)))
        return rb, cols[:self.info.nnz], vals[:self.info.nnz]

    def observe(self, d_u, d_y, n_rhs=1, ld_u=None, ld_y=None, stream=None):
        """y[q, c] = (O u_c)_q on a coarse multi-vector, d_y[q * ld_y + c]; an object of one member.  Asynchronous."""
        self.slod._check(self.lib.slod_lod_observe_multi(self.slod.h, self.r, d_u, n_rhs if ld_u is None else ld_u, n_rhs, d_y,
                                                         n_rhs if ld_y is None else ld_y, stream))

    def observe_ensemble(self, d_u, d_y, n_members=None, first_member=0, ld_u=None, ld_y=None, stream=None):
        """Column m with the values of member first_member + m (n_members defaults to the rest of the object)."""
        K = self.n_members - first_member if n_members is None else n_members
        self.slod._check(self.lib.slod_lod_observe_ensemble(self.slod.h, self.r, first_member, K, d_u, K if ld_u is None else ld_u,
                                                            d_y, K if ld_y is None else ld_y, stream))

    def close(self):
        if self.r:
            self.lib.slod_lod_receivers_destroy(self.r)
            self.r = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ricker(t, f0, t0, amp=1.0):
    """The Ricker wavelet amp (1 - 2 a) exp(-a), a = (pi f0 (t - t0))^2, at the times t: numpy float64, host only."""
    a = (np.pi * np.float64(f0) * (np.asarray(t, dtype=np.float64) - np.float64(t0))) ** 2
    return np.float64(amp) * (1.0 - 2.0 * a) * np.exp(-a)


class Sources:
    """slod_lod_sources: a receivers object applied transposed, b = base + O^T g; source q is receiver q of `recv`, which may
    be closed afterwards.  .info (n_sources, n_members, n_rows_touched, nnz, bytes), .inject(...), .inject_ensemble(...),
    .close()."""

    def __init__(self, slod, recv):
        self.slod, self.lib = slod, slod.lib
        self.s = C.c_void_p()
        slod._check(self.lib.slod_lod_sources_create(slod.h, recv.r if isinstance(recv, Receivers) else recv, C.byref(self.s)))
        self.info = SourcesInfo()
        slod._check(self.lib.slod_lod_sources_get_info(self.s, C.byref(self.info)))
        self.n_src, self.n_members = self.info.n_sources, self.info.n_members
        slod._factors.add(self)                        # the handle closes its objects before itself

    def inject(self, d_g, d_b, n_rhs=1, d_base=None, ld_g=None, ld_base=None, ld_b=None, stream=None):
        """b[r, c] = base[r, c] + (O^T g_c)_r, g of source q at d_g[q * ld_g + c]; d_base None: +0.0; d_b may be d_base.  An
        object of one member.  Asynchronous."""
        self.slod._check(self.lib.slod_lod_inject_multi(self.slod.h, self.s, d_g, n_rhs if ld_g is None else ld_g, n_rhs, d_base,
                                                        n_rhs if ld_base is None else ld_base, d_b, n_rhs if ld_b is None else ld_b,
                                                        stream))

    def inject_ensemble(self, d_g, d_b, n_members=None, first_member=0, d_base=None, ld_g=None, ld_base=None, ld_b=None, stream=None):
        """Column m with the values of member first_member + m (n_members defaults to the rest of the object)."""
        K = self.n_members - first_member if n_members is None else n_members
        self.slod._check(self.lib.slod_lod_inject_ensemble(self.slod.h, self.s, first_member, K, d_g, K if ld_g is None else ld_g,
                                                           d_base, K if ld_base is None else ld_base, d_b,
                                                           K if ld_b is None else ld_b, stream))

    def close(self):
        if self.s:
            self.lib.slod_lod_sources_destroy(self.s)
            self.s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


LodFactor = Factor   # the name of the object in the documents of the LDL^T factor: .inertia(member=0)


def _factor_ptr(f):
    return f.f if isinstance(f, Factor) else f


IRK_GAUSS2, IRK_RADAU2A = 0, 1   # enum slod_irk_scheme


def _irk_scheme(scheme):
    return {"gauss": IRK_GAUSS2, "radau": IRK_RADAU2A}.get(scheme, scheme)


class Slod:
    """Thin OO wrapper over a slod_handle."""

    def __init__(self, nref=0, n_sub=2, oversampling=1, spacedim=1, stabilize=1, reuse_full=0,
                 proj_quirk=0, n_cells=0, n_problems=1, device=0):
        self.lib = load()
        self.cfg = Config(2, spacedim, nref, n_cells, n_sub, oversampling, stabilize, reuse_full,
                          proj_quirk, n_problems, device, 0)
        self.h = C.c_void_p()
        self._factors = weakref.WeakSet()
        rc = self.lib.slod_create(C.byref(self.cfg), C.byref(self.h))
        if rc:
            raise SlodError(rc, self.lib.slod_last_error(None).decode())
        self.N = n_cells if n_cells > 0 else 1 << nref
        self.NE = self.N * n_sub
        self.spacedim = spacedim
        self.num_patches = self.lib.slod_num_patches(self.h)

    def _check(self, rc):
        if rc:
            raise SlodError(rc, self.lib.slod_last_error(self.h).decode())

    def close(self):
        if self.h:
            for f in list(self._factors):
                f.close()
            self.lib.slod_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def patch_layout(self, pid):
        info = PatchInfo()
        self._check(self.lib.slod_patch_layout(self.h, pid, C.byref(info)))
        return info

    def patch_cells(self, pid):
        info = self.patch_layout(pid)
        buf = (C.c_uint32 * (info.mx * info.my))()
        n = self.lib.slod_patch_cells(self.h, pid, buf, len(buf))
        if n < 0:
            self._check(n)
        return list(buf)[:n]

    def patch_dof_permutation(self, pid):
        info = self.patch_layout(pid)
        buf = (C.c_uint32 * info.n_fine)()
        n = self.lib.slod_patch_dof_permutation(self.h, pid, buf, len(buf))
        if n < 0:
            self._check(n)
        return np.array(buf[:n], dtype=np.int64)

    def set_coefficient(self, field, data, problem=0, per_qp=True):
        a = np.ascontiguousarray(data, dtype=np.float64).ravel()
        self._check(self.lib.slod_set_coefficient(self.h, problem, field, a.ctypes.data, 1 if per_qp else 0,
                                                  a.size, 0))

    def set_coefficient_device(self, field, dev_ptr, count, problem=0, per_qp=True):
        self._check(self.lib.slod_set_coefficient(self.h, problem, field, dev_ptr, 1 if per_qp else 0,
                                                  count, 1))

    def plan(self, gids, offsets=None):
        return Plan(self, gids, offsets)

    # ---- refresh after a local coefficient change; d_dirty: device array of num_patches uint32 (raw pointer) ----
    def update_coefficient(self, field, data, d_dirty, problem=0, per_qp=True):
        """set_coefficient that also flags, in d_dirty, the patches whose extent holds a changed fine element."""
        a = np.ascontiguousarray(data, dtype=np.float64).ravel()
        self._check(self.lib.slod_update_coefficient(self.h, problem, field, a.ctypes.data, 1 if per_qp else 0, a.size, 0,
                                                     d_dirty))

    def update_coefficient_device(self, field, dev_ptr, count, d_dirty, problem=0, per_qp=True):
        self._check(self.lib.slod_update_coefficient(self.h, problem, field, dev_ptr, 1 if per_qp else 0, count, 1, d_dirty))

    def dirty_patches(self, d_dirty, count_only=False):
        """Ascending ids of the dirty patches (an int64 array), or their number with count_only.  Synchronises."""
        n = self.lib.slod_dirty_patches(self.h, d_dirty, None, 0)
        if n < 0:
            self._check(n)
        if count_only:
            return n
        buf = np.zeros(max(n, 1), dtype=np.uint32)
        m = self.lib.slod_dirty_patches(self.h, d_dirty, buf.ctypes.data_as(C.POINTER(C.c_uint32)), n)
        if m < 0:
            self._check(m)
        return buf[:m].astype(np.int64)

    def plan_dirty(self, d_dirty, problem=0):
        """The plan that overwrites the dirty patches of the problem's uniform-stride slab in place
        (slod_plan_create_dirty); len(plan.gids) is the C call's return value."""
        return Plan(self, None, dirty=(problem, d_dirty))

    def lod_matrix_update(self, d_dirty, d_basis, d_premult, stride, d_values, ld_m=1, stream=None):
        """Recomputes in place the entries of A_LOD with a dirty row or column.  Asynchronous."""
        self._check(self.lib.slod_lod_matrix_update(self.h, d_dirty, d_basis, d_premult, stride, d_values, ld_m, stream))

    def lod_mass_matrix_update(self, d_dirty, d_basis, stride, d_values, d_rho=None, stream=None):
        """Recomputes in place the entries of M_LOD with a dirty row or column.  Asynchronous."""
        self._check(self.lib.slod_lod_mass_matrix_update(self.h, d_dirty, d_basis, stride, d_rho, d_values, stream))

    # ---- consumers of (phi, psi): the global LOD system (raw device pointers as ints) ----
    def lod_row_capacity(self):
        return self.lib.slod_lod_row_capacity(self.h)

    def lod_pattern(self, pid):
        buf = (C.c_uint32 * self.lod_row_capacity())()
        n = self.lib.slod_lod_pattern(self.h, pid, buf, len(buf))
        if n < 0:
            self._check(n)
        return list(buf)[:n]

    def lod_matrix(self, rows, d_basis, d_premult, stride, d_values, d_cols, stream=None):
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        self._check(self.lib.slod_lod_matrix(self.h, rows.ctypes.data_as(C.POINTER(C.c_uint32)), len(rows), d_basis,
                                             d_premult, stride, d_values, d_cols, stream))

    def lod_rhs(self, rows, d_basis, stride, d_fine_rhs, d_out, stream=None):
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        self._check(self.lib.slod_lod_rhs(self.h, rows.ctypes.data_as(C.POINTER(C.c_uint32)), len(rows), d_basis, stride,
                                          d_fine_rhs, d_out, stream))

    def lod_solve(self, d_values, d_cols, d_rhs, d_u, rel_tol=1e-12, max_iterations=2000):
        res = C.c_double()
        it = self.lib.slod_lod_solve(self.h, d_values, d_cols, d_rhs, d_u, rel_tol, max_iterations, C.byref(res))
        if it < 0:
            self._check(it)
        return it, res.value

    def lod_reconstruct(self, d_basis, stride, d_u, d_fine, stream=None):
        self._check(self.lib.slod_lod_reconstruct(self.h, d_basis, stride, d_u, d_fine, stream))

    # ---- the same three steps for n_rhs load vectors at once.  Fine multi-vectors: field c at + c * ld_fine;
    # coarse multi-vectors interleaved, entry (i, c) at [i * ld + c] (include/slod.h) ----
    def lod_rhs_multi(self, rows, d_basis, stride, d_fine_rhs, ld_fine, n_rhs, d_out, ld_out, stream=None):
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        self._check(self.lib.slod_lod_rhs_multi(self.h, rows.ctypes.data_as(C.POINTER(C.c_uint32)), len(rows), d_basis,
                                                stride, d_fine_rhs, ld_fine, n_rhs, d_out, ld_out, stream))

    def lod_solve_multi(self, d_values, d_cols, d_rhs, ld_rhs, n_rhs, d_u, ld_u, rel_tol=1e-12, max_iterations=2000):
        """Returns (iterations, rel_residual), one entry per column; max(iterations) is the C call's return value."""
        its = np.zeros(max(n_rhs, 1), dtype=np.intc)
        res = np.zeros(max(n_rhs, 1))
        rc = self.lib.slod_lod_solve_multi(self.h, d_values, d_cols, d_rhs, ld_rhs, n_rhs, d_u, ld_u, rel_tol,
                                           max_iterations, its.ctypes.data_as(C.POINTER(C.c_int)), _dp(res))
        if rc < 0:
            self._check(rc)
        return its[:n_rhs], res[:n_rhs]

    def lod_reconstruct_multi(self, d_basis, stride, d_u, ld_u, n_rhs, d_fine, ld_fine, stream=None):
        self._check(self.lib.slod_lod_reconstruct_multi(self.h, d_basis, stride, d_u, ld_u, n_rhs, d_fine, ld_fine, stream))

    # ---- the L2 side: M_LOD = C^T M_rho C, products and combinations of block-row matrices, theta time steps ----
    def lod_mass_matrix(self, rows, d_basis, stride, d_values, d_cols, d_rho=None, stream=None):
        """Block rows of M_LOD in the layout of lod_matrix (d_rho: device [NE][NE] per fine element, None = 1)."""
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        self._check(self.lib.slod_lod_mass_matrix(self.h, rows.ctypes.data_as(C.POINTER(C.c_uint32)), len(rows), d_basis,
                                                  stride, d_rho, d_values, d_cols, stream))

    def lod_apply(self, d_values, d_cols, d_x, d_y, n_rhs=1, ld_x=None, ld_y=None, stream=None):
        """Y = A X on a full set of block rows; coarse multi-vectors, ld defaults to n_rhs.  Asynchronous."""
        self._check(self.lib.slod_lod_apply_multi(self.h, d_values, d_cols, d_x, n_rhs if ld_x is None else ld_x, n_rhs,
                                                  d_y, n_rhs if ld_y is None else ld_y, stream))

    def lod_matrix_combine(self, alpha, d_a, beta, d_b, d_out, stream=None):
        """out = alpha * A + beta * B on two values arrays of one pattern (out may be an input).  Asynchronous."""
        self._check(self.lib.slod_lod_matrix_combine(self.h, alpha, d_a, beta, d_b, d_out, stream))

    def lod_theta_steps(self, d_stiffness, d_mass, d_cols, dt, theta, n_steps, d_u, n_rhs=1, ld_u=None, d_load=None,
                        ld_load=None, load_step_stride=0, rel_tol=1e-12, max_iterations=2000):
        """n_steps of the theta scheme for M u' + A u = b(t) on d_u in place.  Returns (iterations, rel_residual),
        one entry per step; max(iterations) is the C call's return value."""
        its = np.zeros(max(n_steps, 1), dtype=np.intc)
        res = np.zeros(max(n_steps, 1))
        rc = self.lib.slod_lod_theta_steps(self.h, d_stiffness, d_mass, d_cols, dt, theta, n_steps, n_rhs, d_u,
                                           n_rhs if ld_u is None else ld_u, d_load, n_rhs if ld_load is None else ld_load,
                                           load_step_stride, rel_tol, max_iterations,
                                           its.ctypes.data_as(C.POINTER(C.c_int)), _dp(res))
        if rc < 0:
            self._check(rc)
        return its[:n_steps], res[:n_steps]

    # ---- the eigenvalue problem A_LOD u = lambda M_LOD u ----
    def lod_matrix_symmetrize(self, d_values, d_cols, d_out, stream=None):
        """out = 0.5 * (A + A^T) on a full set of block rows, bit-symmetric; not in place.  Asynchronous."""
        self._check(self.lib.slod_lod_matrix_symmetrize(self.h, d_values, d_cols, d_out, stream))

    def lod_eigs(self, d_stiffness, d_mass, d_cols, n_eig, d_x, n_block=None, ld_x=None, start=0, tol=1e-10, max_outer=200,
                 inner_rel_tol=1e-12, inner_max_iterations=2000):
        """The lowest n_eig eigenpairs of the symmetric pencil (A, M) by block inverse iteration with Rayleigh-Ritz on
        n_block columns (default: n_eig and a few guard columns); d_x receives the M-orthonormal block.  Returns
        (eigenvalues[n_block], residuals[n_block], inner_iterations[outer]); len(inner_iterations) is the C call's
        return value.  The guard columns n_eig .. n_block-1 are less converged."""
        if n_block is None:
            n_block = min(64, self.num_patches * self.spacedim, n_eig + max(4, n_eig // 2))
        lam = np.zeros(max(n_block, 1))
        res = np.zeros(max(n_block, 1))
        its = np.zeros(max(max_outer, 1), dtype=np.intc)
        rc = self.lib.slod_lod_eigs(self.h, d_stiffness, d_mass, d_cols, n_eig, n_block, start, d_x,
                                    n_block if ld_x is None else ld_x, tol, max_outer, inner_rel_tol, inner_max_iterations,
                                    _dp(lam), _dp(res), its.ctypes.data_as(C.POINTER(C.c_int)))
        if rc < 0:
            self._check(rc)
        return lam[:n_block], res[:n_block], its[:rc]

    # ---- second-order time stepping: M u'' + C u' + A u = b(t), C = damp_mass M + damp_stiff A ----
    def lod_inner(self, d_values, d_cols, d_x, d_y, n_rhs=1, ld_x=None, ld_y=None, stream=None):
        """out[c] = x_c^T (A y_c) per column, in a fixed summation order; d_x may be d_y.  Returns an array [n_rhs]."""
        out = np.zeros(max(n_rhs, 1))
        self._check(self.lib.slod_lod_inner_multi(self.h, d_values, d_cols, d_x, n_rhs if ld_x is None else ld_x, d_y,
                                                  n_rhs if ld_y is None else ld_y, n_rhs, _dp(out), stream))
        return out[:n_rhs]

    def lod_newmark_accel(self, d_stiffness, d_mass, d_cols, d_u, d_v, d_a, n_rhs=1, ld_u=None, ld_v=None, ld_a=None,
                          d_load=None, ld_load=None, damp_mass=0.0, damp_stiff=0.0, rel_tol=1e-12, max_iterations=2000,
                          d_damping=None):
        """d_a = the solution of M a = b^0 - A (u + damp_stiff v) - damp_mass M v per column.  Returns
        (iterations, rel_residual), one entry per column; max(iterations) is the C call's return value.
        d_damping: the third damping matrix D (slod_lod_newmark_accel_damped), - D v joins the right-hand side."""
        its = np.zeros(max(n_rhs, 1), dtype=np.intc)
        res = np.zeros(max(n_rhs, 1))
        fn, mats = (self.lib.slod_lod_newmark_accel, (d_stiffness, d_mass)) if d_damping is None else \
            (self.lib.slod_lod_newmark_accel_damped, (d_stiffness, d_mass, d_damping))
        rc = fn(self.h, *mats, d_cols, damp_mass, damp_stiff, n_rhs, d_u,
                n_rhs if ld_u is None else ld_u, d_v, n_rhs if ld_v is None else ld_v, d_load,
                n_rhs if ld_load is None else ld_load, d_a, n_rhs if ld_a is None else ld_a,
                rel_tol, max_iterations, its.ctypes.data_as(C.POINTER(C.c_int)), _dp(res))
        if rc < 0:
            self._check(rc)
        return its[:n_rhs], res[:n_rhs]

    def lod_newmark_steps(self, d_stiffness, d_mass, d_cols, dt, n_steps, d_u, d_v, d_a, beta=0.25, gamma=0.5, n_rhs=1,
                          ld_u=None, ld_v=None, ld_a=None, d_load=None, ld_load=None, load_step_stride=0, damp_mass=0.0,
                          damp_stiff=0.0, rel_tol=1e-12, max_iterations=2000, energies=True, d_damping=None):
        """n_steps of Newmark-beta on d_u, d_v, d_a in place.  Returns (iterations, rel_residual, kinetic, potential):
        the first two with one entry per step, the energies as arrays [n_steps + 1, n_rhs] (row 0: the entry state), or
        None for both with energies=False; max(iterations) is the C call's return value.
        d_damping: the third damping matrix D (slod_lod_newmark_steps_damped)."""
        its = np.zeros(max(n_steps, 1), dtype=np.intc)
        res = np.zeros(max(n_steps, 1))
        shape = (max(n_steps, 0) + 1, max(n_rhs, 1))
        kin, pot = (np.zeros(shape), np.zeros(shape)) if energies else (None, None)
        fn, mats = (self.lib.slod_lod_newmark_steps, (d_stiffness, d_mass)) if d_damping is None else \
            (self.lib.slod_lod_newmark_steps_damped, (d_stiffness, d_mass, d_damping))
        rc = fn(self.h, *mats, d_cols, dt, beta, gamma, damp_mass, damp_stiff,
                n_steps, n_rhs, d_u, n_rhs if ld_u is None else ld_u, d_v,
                n_rhs if ld_v is None else ld_v, d_a, n_rhs if ld_a is None else ld_a, d_load,
                n_rhs if ld_load is None else ld_load, load_step_stride, rel_tol, max_iterations,
                its.ctypes.data_as(C.POINTER(C.c_int)), _dp(res),
                _dp(kin) if energies else None, _dp(pot) if energies else None)
        if rc < 0:
            self._check(rc)
        return its[:n_steps], res[:n_steps], kin, pot

    # ---- the direct solver: banded Cholesky of a full set of block rows, and the time loops on a factor ----
    def lod_factor(self, d_values, d_cols):
        """The Cholesky factor of a symmetric positive definite matrix in block rows: an object with .info (n,
        half_bandwidth, block, bytes, min_pivot, max_pivot), .solve(d_rhs, d_u, n_rhs, ...) and .close().
        SlodError(-5) when a pivot is not positive."""
        return Factor(self, d_values, d_cols)

    def lod_factor_ldl(self, d_values, d_cols):
        """The LDL^T factor (no pivoting) of a symmetric matrix in block rows, indefinite or not: a Factor whose .info has
        the signed range of D and whose .inertia() counts the signs of D and measures the growth."""
        return Factor(self, d_values, d_cols, ldl=True)

    def lod_factor_zldl(self, d_a, d_b, d_cols, alpha, beta):
        """The complex symmetric LDL^T factors of S_k = alpha[k] A + beta[k] B (no pivoting), one member per pair of
        complex coefficients: a ComplexFactor with .info, .inertia(member), .solve_complex(...) and .close()."""
        return ComplexFactor(self, d_a, d_b, d_cols, alpha, beta)

    def lod_factor_zldl3(self, d_a, d_b, d_c, d_cols, alpha, beta, gamma):
        """lod_factor_zldl with a third term: S_k = alpha[k] A + beta[k] B + gamma[k] C (slod_lod_factor_create_zldl3)."""
        return ComplexFactor(self, d_a, d_b, d_cols, alpha, beta, d_c=d_c, gamma=gamma)

    def lod_factor_zldl_ensemble(self, d_a, d_b, d_cols, n_members, alpha, beta, ld_a_m=None, ld_b_m=None):
        """lod_factor_zldl on ensemble matrices of n_members members: the factor member j = k * n_members + m is
        alpha[k] A_m + beta[k] B_m.  A ComplexFactor; solve_complex(..., rhs_members=) maps the members to rhs columns."""
        return ComplexFactor(self, d_a, d_b, d_cols, alpha, beta, matrix_members=n_members, ld_a_m=ld_a_m, ld_b_m=ld_b_m)

    def lod_harmonic_response_ensemble(self, d_stiffness, d_mass, d_cols, n_members, omega, d_load_re, d_load_im, d_u_re, d_u_im,
                                       n_rhs=1, damp_mass=0.0, damp_stiff=0.0, ld_a_m=None, ld_m_m=None, ld_load=None, ld_u=None):
        """lod_harmonic_response for the n_members = K members of an ensemble matrix pair: (frequency k, member m, load
        column c) is column (k K + m) * n_rhs + c of (d_u_re, d_u_im); member m's loads are the columns m * n_rhs + c of the
        load.  Returns (rel_residual[F, K, n_rhs], growth[F, K], quantities[F, K, n_rhs, 4]) with
        quantities = (u^H M u, u^H A u, Re u^H b, Im u^H b)."""
        w = np.ascontiguousarray(np.atleast_1d(omega), dtype=np.float64)
        F, K, n = len(w), max(n_members, 1), max(n_rhs, 1)
        res, growth, q = np.zeros((F, K, n)), np.zeros((F, K)), np.zeros((F, K, n, 4))
        self._check(self.lib.slod_lod_harmonic_response_ensemble(
            self.h, d_stiffness, n_members if ld_a_m is None else ld_a_m, d_mass, n_members if ld_m_m is None else ld_m_m,
            d_cols, n_members, damp_mass, damp_stiff, _dp(w), F, d_load_re, d_load_im,
            n_members * n_rhs if ld_load is None else ld_load, n_rhs, d_u_re, d_u_im,
            F * n_members * n_rhs if ld_u is None else ld_u, _dp(res), _dp(growth), _dp(q)))
        return res, growth, q

    def lod_harmonic_response(self, d_stiffness, d_mass, d_cols, omega, d_load_re, d_load_im, d_u_re, d_u_im, n_rhs=1,
                              damp_mass=0.0, damp_stiff=0.0, ld_load=None, ld_u=None, d_damping=None):
        """S(omega_k) u = load for every frequency of omega, S = (1 + i omega damp_stiff) A + (i omega damp_mass - omega^2) M;
        frequency k writes the columns k * n_rhs .. of (d_u_re, d_u_im).  d_load_im None: a real load.  Returns
        (rel_residual[n_freq, n_rhs], growth[n_freq]).
        d_damping: the third damping matrix D (slod_lod_harmonic_response_damped), S gains i omega D; the call then also
        returns quantities[n_freq, n_rhs, 5] = (u^H M u, u^H A u, u^H D u, Re u^H b, Im u^H b)."""
        w = np.ascontiguousarray(np.atleast_1d(omega), dtype=np.float64)
        res, growth = np.zeros((len(w), max(n_rhs, 1))), np.zeros(len(w))
        if d_damping is not None:
            q = np.zeros((len(w), max(n_rhs, 1), 5))
            self._check(self.lib.slod_lod_harmonic_response_damped(
                self.h, d_stiffness, d_mass, d_damping, d_cols, damp_mass, damp_stiff, _dp(w), len(w), d_load_re, d_load_im,
                n_rhs if ld_load is None else ld_load, n_rhs, d_u_re, d_u_im, len(w) * n_rhs if ld_u is None else ld_u,
                _dp(res), _dp(growth), _dp(q)))
            return res, growth, q
        self._check(self.lib.slod_lod_harmonic_response(
            self.h, d_stiffness, d_mass, d_cols, damp_mass, damp_stiff, _dp(w), len(w), d_load_re, d_load_im,
            n_rhs if ld_load is None else ld_load, n_rhs, d_u_re, d_u_im, len(w) * n_rhs if ld_u is None else ld_u,
            _dp(res), _dp(growth)))
        return res, growth

    def lod_theta_steps_direct(self, factor, d_stiffness, d_cols, dt, theta, n_steps, d_u, n_rhs=1, ld_u=None, d_load=None,
                               ld_load=None, load_step_stride=0):
        """lod_theta_steps on the factor of S = M + theta dt A (lod_matrix_combine(1, M, theta * dt, A))."""
        self._check(self.lib.slod_lod_theta_steps_direct(self.h, _factor_ptr(factor), d_stiffness, d_cols, dt, theta, n_steps,
                                                         n_rhs, d_u, n_rhs if ld_u is None else ld_u, d_load,
                                                         n_rhs if ld_load is None else ld_load, load_step_stride))

    def lod_newmark_accel_direct(self, factor, d_stiffness, d_mass, d_cols, d_u, d_v, d_a, n_rhs=1, ld_u=None, ld_v=None,
                                 ld_a=None, d_load=None, ld_load=None, damp_mass=0.0, damp_stiff=0.0, d_damping=None):
        """lod_newmark_accel on the factor of M; d_damping: slod_lod_newmark_accel_damped_direct."""
        fn, mats = (self.lib.slod_lod_newmark_accel_direct, (d_stiffness, d_mass)) if d_damping is None else \
            (self.lib.slod_lod_newmark_accel_damped_direct, (d_stiffness, d_mass, d_damping))
        self._check(fn(
            self.h, _factor_ptr(factor), *mats, d_cols, damp_mass, damp_stiff, n_rhs, d_u,
            n_rhs if ld_u is None else ld_u, d_v, n_rhs if ld_v is None else ld_v, d_load,
            n_rhs if ld_load is None else ld_load, d_a, n_rhs if ld_a is None else ld_a))

    def lod_newmark_steps_direct(self, factor, d_stiffness, d_mass, d_cols, dt, n_steps, d_u, d_v, d_a, beta=0.25, gamma=0.5,
                                 n_rhs=1, ld_u=None, ld_v=None, ld_a=None, d_load=None, ld_load=None, load_step_stride=0,
                                 damp_mass=0.0, damp_stiff=0.0, energies=True, d_damping=None):
        """lod_newmark_steps on the factor of S = (1 + gamma dt damp_mass) M + (beta dt^2 + gamma dt damp_stiff) A.
        Returns (kinetic, potential) as arrays [n_steps + 1, n_rhs], or (None, None) with energies=False.
        d_damping: the third damping matrix D (slod_lod_newmark_steps_damped_direct) on the factor of S + gamma dt D."""
        shape = (max(n_steps, 0) + 1, max(n_rhs, 1))
        kin, pot = (np.zeros(shape), np.zeros(shape)) if energies else (None, None)
        fn, mats = (self.lib.slod_lod_newmark_steps_direct, (d_stiffness, d_mass)) if d_damping is None else \
            (self.lib.slod_lod_newmark_steps_damped_direct, (d_stiffness, d_mass, d_damping))
        self._check(fn(
            self.h, _factor_ptr(factor), *mats, d_cols, dt, beta, gamma, damp_mass, damp_stiff, n_steps, n_rhs,
            d_u, n_rhs if ld_u is None else ld_u, d_v, n_rhs if ld_v is None else ld_v, d_a, n_rhs if ld_a is None else ld_a,
            d_load, n_rhs if ld_load is None else ld_load, load_step_stride, _dp(kin) if energies else None,
            _dp(pot) if energies else None))
        return kin, pot

    # ---- two-stage implicit Runge-Kutta on a member of a complex factor: one complex solve per step ----
    def lod_irk_coefficients(self, scheme, order, dt, damp_mass=0.0, damp_stiff=0.0):
        """(alpha, beta), complex, of the step matrix S = alpha A + beta M of scheme IRK_GAUSS2 / IRK_RADAU2A (or "gauss" /
        "radau") for lod_factor_zldl(sym(A), M, cols, alpha, beta); order 1: heat, 2: wave."""
        a, b = np.zeros(2), np.zeros(2)
        rc = self.lib.slod_lod_irk_coefficients(_irk_scheme(scheme), order, dt, damp_mass, damp_stiff, _dp(a), _dp(b))
        if rc:
            raise SlodError(rc, self.lib.slod_last_error(None).decode())
        return complex(a[0], a[1]), complex(b[0], b[1])

    def lod_irk_damping_coefficient(self, scheme, dt):
        """gamma = dt lambda, complex: the coefficient of D in the step matrix of the damped wave, for lod_factor_zldl3 with
        the pair of lod_irk_coefficients(scheme, 2, ..)."""
        g = np.zeros(2)
        rc = self.lib.slod_lod_irk_damping_coefficient(_irk_scheme(scheme), dt, _dp(g))
        if rc:
            raise SlodError(rc, self.lib.slod_last_error(None).decode())
        return complex(g[0], g[1])

    def lod_irk_heat_steps(self, factor, scheme, d_stiffness, d_cols, dt, n_steps, d_u, n_rhs=1, member=0, ld_u=None,
                           d_load=None, ld_load=None, load_stage_stride=0):
        """n_steps of the two-stage scheme for M u' + A u = b(t) on d_u in place, on member `member` of the complex
        factor of S = M + dt lambda A (lod_irk_coefficients).  Stage i of step k reads the load at
        d_load + (2 k + i) * load_stage_stride doubles."""
        self._check(self.lib.slod_lod_irk_heat_steps_direct(
            self.h, _factor_ptr(factor), member, _irk_scheme(scheme), d_stiffness, d_cols, dt, n_steps, n_rhs, d_u,
            n_rhs if ld_u is None else ld_u, d_load, n_rhs if ld_load is None else ld_load, load_stage_stride))

    def lod_irk_wave_steps(self, factor, scheme, d_stiffness, d_mass, d_cols, dt, n_steps, d_u, d_v, n_rhs=1, member=0,
                           ld_u=None, ld_v=None, d_load=None, ld_load=None, load_stage_stride=0, damp_mass=0.0,
                           damp_stiff=0.0, energies=True, d_damping=None):
        """n_steps of the two-stage scheme for M u'' + C u' + A u = b(t) on d_u, d_v in place, on member `member` of the
        complex factor of lod_irk_coefficients(scheme, 2, dt, damp_mass, damp_stiff).  Returns (kinetic, potential) as
        arrays [n_steps + 1, n_rhs], or (None, None) with energies=False.
        d_damping: the third damping matrix D (slod_lod_irk_wave_steps_damped_direct), on a member of lod_factor_zldl3 with
        gamma = lod_irk_damping_coefficient(scheme, dt)."""
        shape = (max(n_steps, 0) + 1, max(n_rhs, 1))
        kin, pot = (np.zeros(shape), np.zeros(shape)) if energies else (None, None)
        fn, mats = (self.lib.slod_lod_irk_wave_steps_direct, (d_stiffness, d_mass)) if d_damping is None else \
            (self.lib.slod_lod_irk_wave_steps_damped_direct, (d_stiffness, d_mass, d_damping))
        self._check(fn(
            self.h, _factor_ptr(factor), member, _irk_scheme(scheme), *mats, d_cols, dt, damp_mass, damp_stiff,
            n_steps, n_rhs, d_u, n_rhs if ld_u is None else ld_u, d_v, n_rhs if ld_v is None else ld_v, d_load,
            n_rhs if ld_load is None else ld_load, load_stage_stride, _dp(kin) if energies else None,
            _dp(pot) if energies else None))
        return kin, pot

    def lod_irk_heat_steps_ensemble(self, factor, scheme, d_stiffness, d_cols, dt, n_steps, n_members, d_u, first_member=0,
                                    ld_a_m=None, ld_u=None, d_load=None, ld_load=None, load_stage_stride=0):
        """lod_irk_heat_steps with a matrix, a factor member and a column per ensemble member: column m of d_u is advanced
        on factor member first_member + m with member m of the ensemble matrix d_stiffness.  Stage i of step k, member m,
        row r reads the load at d_load[(2 k + i) * load_stage_stride + r * ld_load + m]."""
        K = n_members
        self._check(self.lib.slod_lod_irk_heat_steps_ensemble_direct(
            self.h, _factor_ptr(factor), first_member, _irk_scheme(scheme), d_stiffness, K if ld_a_m is None else ld_a_m,
            d_cols, dt, n_steps, K, d_u, K if ld_u is None else ld_u, d_load, K if ld_load is None else ld_load,
            load_stage_stride))

    def lod_irk_wave_steps_ensemble(self, factor, scheme, d_stiffness, d_mass, d_cols, dt, n_steps, n_members, d_u, d_v,
                                    first_member=0, ld_a_m=None, ld_m_m=None, ld_u=None, ld_v=None, d_load=None, ld_load=None,
                                    load_stage_stride=0, damp_mass=0.0, damp_stiff=0.0, energies=True):
        """lod_irk_wave_steps with a matrix pair, a factor member and a column per ensemble member.  Returns
        (kinetic, potential) as arrays [n_steps + 1, n_members], or (None, None) with energies=False."""
        K = n_members
        shape = (max(n_steps, 0) + 1, max(K, 1))
        kin, pot = (np.zeros(shape), np.zeros(shape)) if energies else (None, None)
        self._check(self.lib.slod_lod_irk_wave_steps_ensemble_direct(
            self.h, _factor_ptr(factor), first_member, _irk_scheme(scheme), d_stiffness, K if ld_a_m is None else ld_a_m,
            d_mass, K if ld_m_m is None else ld_m_m, d_cols, dt, damp_mass, damp_stiff, n_steps, K, d_u,
            K if ld_u is None else ld_u, d_v, K if ld_v is None else ld_v, d_load, K if ld_load is None else ld_load,
            load_stage_stride, _dp(kin) if energies else None, _dp(pot) if energies else None))
        return kin, pot

    # ---- receivers: (C u)(x) at a few points, as a product and as a trace of the time loops ----
    def lod_receiver_capacity(self):
        return self.lib.slod_lod_receiver_capacity(self.h)

    def lod_receiver_pattern(self, node):
        """The columns p * s + d of the row of a term at the fine node `node`, in row order (host only)."""
        buf = (C.c_uint32 * self.lod_receiver_capacity())()
        n = self.lib.slod_lod_receiver_pattern(self.h, node, buf, len(buf))
        if n < 0:
            self._check(n)
        return list(buf)[:n]

    def lod_receivers(self, receivers, d_basis, stride, n_members=1, member_stride=None, raw=False):
        """The rows of a set of receivers (each a sequence of terms (node, comp, weight); point_terms gives the four of a
        point) from the basis slab, or from the n_members slabs of an ensemble: a Receivers object."""
        return Receivers(self, receivers, d_basis, stride, n_members, member_stride, raw)

    def lod_time_record(self, recv, trace_ptr, capacity=0, what=RECORD_U, every=1, ld_trace=None, record_stride=None, columns=1):
        """Arms the record of the NEXT stepper call on this handle (one-shot): record j, quantity w (u before v), receiver q,
        column c at trace_ptr[j * record_stride + (w * n_recv + q) * ld_trace + c] doubles.  ld_trace defaults to `columns`
        (n_rhs or n_members of the stepper), record_stride to n_quantities * n_recv * ld_trace.  recv=None disarms."""
        if recv is None:
            self._check(self.lib.slod_lod_time_record_arm(self.h, None))
            return None
        ld = columns if ld_trace is None else ld_trace
        nq = 2 if what == (RECORD_U | RECORD_V) else 1
        rec = TimeRecord(recv.r if isinstance(recv, Receivers) else recv, what, every, trace_ptr, ld,
                         nq * recv.n_recv * ld if record_stride is None else record_stride, capacity)
        self._check(self.lib.slod_lod_time_record_arm(self.h, C.byref(rec)))
        return rec

    # ---- sources: point forces with a time signal, as a product and as a load of the time loops ----
    def lod_sources(self, recv):
        """The sources of a Receivers object (source q is receiver q): a Sources object."""
        return Sources(self, recv)

    def lod_time_source(self, src, signal_ptr, n_samples=0, ld_signal=None, sample_stride=None, columns=1):
        """Arms the source of the NEXT stepper call on this handle (one-shot): its load is d_load + O^T g, sample j, source q,
        column c at signal_ptr[j * sample_stride + q * ld_signal + c] doubles; theta and Newmark loops read the samples
        0 .. n_steps, IRK loops the samples 2 k + i of stage i of step k.  ld_signal defaults to `columns` (n_rhs or n_members
        of the stepper), sample_stride to n_sources * ld_signal.  src=None disarms."""
        if src is None:
            self._check(self.lib.slod_lod_time_source_arm(self.h, None))
            return
        ld = columns if ld_signal is None else ld_signal
        ts = TimeSource(src.s if isinstance(src, Sources) else src, signal_ptr, ld,
                        src.n_src * ld if sample_stride is None else sample_stride, n_samples)
        self._check(self.lib.slod_lod_time_source_arm(self.h, C.byref(ts)))
        return ts

    # ---- the LOD systems of a coefficient ensemble: member k = problem k of the handle = column k of the coarse
    # multi-vectors; matrix values member-minor, entry e of member k at [e * ld_m + k] (include/slod.h) ----
    def lod_matrix_ensemble(self, d_basis, d_premult, stride, n_members, d_values, d_cols, member_stride=None, ld_m=None,
                            stream=None):
        """Block rows of every member on the shared pattern; member_stride defaults to num_patches * stride, ld_m to
        n_members.  Asynchronous."""
        self._check(self.lib.slod_lod_matrix_ensemble(
            self.h, d_basis, d_premult, stride, self.num_patches * stride if member_stride is None else member_stride,
            n_members, d_values, n_members if ld_m is None else ld_m, d_cols, stream))

    def lod_rhs_ensemble(self, d_basis, stride, n_members, d_fine_rhs, d_out, ld_fine=0, member_stride=None, ld_out=None,
                         stream=None):
        """C_k^T f_k per member; ld_fine = 0: one load shared by all members.  Asynchronous."""
        self._check(self.lib.slod_lod_rhs_ensemble(
            self.h, d_basis, stride, self.num_patches * stride if member_stride is None else member_stride, n_members,
            d_fine_rhs, ld_fine, d_out, n_members if ld_out is None else ld_out, stream))

    def lod_apply_ensemble(self, d_values, d_cols, d_x, d_y, n_members, ld_m=None, ld_x=None, ld_y=None, stream=None):
        """Y_k = A_k X_k; every ld defaults to n_members.  Asynchronous."""
        self._check(self.lib.slod_lod_apply_ensemble(
            self.h, d_values, n_members if ld_m is None else ld_m, d_cols, d_x, n_members if ld_x is None else ld_x,
            n_members, d_y, n_members if ld_y is None else ld_y, stream))

    def lod_solve_ensemble(self, d_values, d_cols, d_rhs, d_u, n_members, ld_m=None, ld_rhs=None, ld_u=None, rel_tol=1e-12,
                           max_iterations=2000):
        """A_k u_k = rhs_k for every member.  Returns (iterations, rel_residual), one entry per member;
        max(iterations) is the C call's return value."""
        its = np.zeros(max(n_members, 1), dtype=np.intc)
        res = np.zeros(max(n_members, 1))
        rc = self.lib.slod_lod_solve_ensemble(
            self.h, d_values, n_members if ld_m is None else ld_m, d_cols, d_rhs, n_members if ld_rhs is None else ld_rhs,
            n_members, d_u, n_members if ld_u is None else ld_u, rel_tol, max_iterations,
            its.ctypes.data_as(C.POINTER(C.c_int)), _dp(res))
        if rc < 0:
            self._check(rc)
        return its[:n_members], res[:n_members]

    def lod_reconstruct_ensemble(self, d_basis, stride, n_members, d_u, d_fine, ld_fine=None, member_stride=None, ld_u=None,
                                 stream=None):
        """Field k of d_fine = C_k u_k; ld_fine defaults to the length of a fine field.  Asynchronous."""
        field = (self.NE + 1) ** 2 * self.spacedim
        self._check(self.lib.slod_lod_reconstruct_ensemble(
            self.h, d_basis, stride, self.num_patches * stride if member_stride is None else member_stride, n_members,
            d_u, n_members if ld_u is None else ld_u, d_fine, field if ld_fine is None else ld_fine, stream))

    def ensemble_moments(self, d_fields, n_members, count, d_mean, d_var=None, ld_fine=None, stream=None):
        """Mean and unbiased variance over the members of `count` entries per field; ld_fine defaults to count.
        Asynchronous."""
        self._check(self.lib.slod_ensemble_moments(self.h, d_fields, count if ld_fine is None else ld_fine, n_members, count,
                                                   d_mean, d_var, stream))

    # ---- the L2 side and the direct solver of an ensemble: a factor per member, the theta scheme with a column per member ----
    def lod_mass_matrix_ensemble(self, d_basis, stride, n_members, d_values, d_cols, d_rho=None, ld_rho=0, member_stride=None,
                                 ld_m=None, stream=None):
        """Block rows of M_LOD of every member; d_rho None = 1, ld_rho = 0: one density for all members.  Asynchronous."""
        self._check(self.lib.slod_lod_mass_matrix_ensemble(
            self.h, d_basis, stride, self.num_patches * stride if member_stride is None else member_stride, n_members, d_rho,
            ld_rho, d_values, n_members if ld_m is None else ld_m, d_cols, stream))

    def lod_matrix_symmetrize_ensemble(self, d_values, d_cols, n_members, d_out, ld_in=None, ld_out=None, stream=None):
        """out_k = 0.5 * (A_k + A_k^T) per member; not in place.  Asynchronous."""
        self._check(self.lib.slod_lod_matrix_symmetrize_ensemble(self.h, d_values, n_members if ld_in is None else ld_in, d_cols,
                                                                 n_members, d_out, n_members if ld_out is None else ld_out, stream))

    def lod_matrix_combine_ensemble(self, alpha, d_a, beta, d_b, n_members, d_out, ld_a=None, ld_b=None, ld_out=None, stream=None):
        """out_k = alpha * A_k + beta * B_k per member (out may be an input of the same ld).  Asynchronous."""
        self._check(self.lib.slod_lod_matrix_combine_ensemble(
            self.h, alpha, d_a, n_members if ld_a is None else ld_a, beta, d_b, n_members if ld_b is None else ld_b, n_members,
            d_out, n_members if ld_out is None else ld_out, stream))

    def lod_factor_ensemble(self, d_values, d_cols, n_members, ld_m=None):
        """The Cholesky factors of the members of an ensemble matrix in one object (EnsembleFactor)."""
        return EnsembleFactor(self, d_values, d_cols, n_members, ld_m)

    def lod_factor_ldl_ensemble(self, d_values, d_cols, n_members, ld_m=None):
        """The LDL^T factors of the members of an ensemble matrix in one object (EnsembleFactor, .inertia(member))."""
        return EnsembleFactor(self, d_values, d_cols, n_members, ld_m, ldl=True)

    # ---- CG preconditioned by a banded factor of a nearby matrix (stale after a refresh, shared by an ensemble) ----
    def _precond_result(self, rc, its, res, n):
        """(iterations, rel_residual) per column; a breakdown raises SlodError(-5) that carries both arrays."""
        if rc < 0:
            err = SlodError(rc, self.lib.slod_last_error(self.h).decode())
            err.iterations, err.rel_residual = its[:max(n, 0)].copy(), res[:max(n, 0)].copy()
            raise err
        return its[:n], res[:n]

    def lod_solve_multi_precond(self, factor, d_values, d_cols, d_rhs, ld_rhs, n_rhs, d_u, ld_u, rel_tol=1e-12,
                                max_iterations=2000):
        """A u_c = rhs_c by CG with z = P^-1 r on `factor` (one member, for all columns).  Returns (iterations,
        rel_residual), one entry per column, the device's counters."""
        its = np.zeros(max(n_rhs, 1), dtype=np.intc)
        res = np.zeros(max(n_rhs, 1))
        rc = self.lib.slod_lod_solve_multi_precond(self.h, _factor_ptr(factor), d_values, d_cols, d_rhs, ld_rhs, n_rhs, d_u, ld_u,
                                                   rel_tol, max_iterations, its.ctypes.data_as(C.POINTER(C.c_int)), _dp(res))
        return self._precond_result(rc, its, res, n_rhs)

    def lod_solve_ensemble_precond(self, factor, d_values, d_cols, d_rhs, d_u, n_members, ld_m=None, ld_rhs=None, ld_u=None,
                                   rel_tol=1e-12, max_iterations=2000):
        """A_k u_k = rhs_k for every member by CG preconditioned by `factor`: of one member (shared by all) or of n_members
        members (member k for column k).  Returns (iterations, rel_residual), one entry per member."""
        its = np.zeros(max(n_members, 1), dtype=np.intc)
        res = np.zeros(max(n_members, 1))
        rc = self.lib.slod_lod_solve_ensemble_precond(
            self.h, _factor_ptr(factor), d_values, n_members if ld_m is None else ld_m, d_cols, d_rhs,
            n_members if ld_rhs is None else ld_rhs, n_members, d_u, n_members if ld_u is None else ld_u, rel_tol, max_iterations,
            its.ctypes.data_as(C.POINTER(C.c_int)), _dp(res))
        return self._precond_result(rc, its, res, n_members)

    def lod_theta_steps_ensemble_direct(self, factor, d_stiffness, d_cols, dt, theta, n_steps, n_members, d_u, ld_m=None,
                                        ld_u=None, d_load=None, ld_load=None, load_step_stride=0):
        """lod_theta_steps_direct with a column, a matrix and a factor per member; the factor is that of
        lod_matrix_combine_ensemble(1, M, theta * dt, A)."""
        self._check(self.lib.slod_lod_theta_steps_ensemble_direct(
            self.h, _factor_ptr(factor), d_stiffness, n_members if ld_m is None else ld_m, d_cols, dt, theta, n_steps, n_members,
            d_u, n_members if ld_u is None else ld_u, d_load, n_members if ld_load is None else ld_load, load_step_stride))

    # ---- the wave equation on an ensemble: Newmark with a column, two matrices and a factor per member ----
    def lod_inner_ensemble(self, d_values, d_cols, d_x, d_y, n_members, ld_m=None, ld_x=None, ld_y=None, stream=None):
        """out[k] = x_k^T (A_k y_k) with member k's matrix; d_x may be d_y.  Returns an array [n_members]."""
        out = np.zeros(max(n_members, 1))
        self._check(self.lib.slod_lod_inner_ensemble(
            self.h, d_values, n_members if ld_m is None else ld_m, d_cols, d_x, n_members if ld_x is None else ld_x, d_y,
            n_members if ld_y is None else ld_y, n_members, _dp(out), stream))
        return out[:n_members]

    def lod_newmark_accel_ensemble_direct(self, factor, d_stiffness, d_mass, d_cols, n_members, d_u, d_v, d_a, ld_a_m=None,
                                          ld_m_m=None, ld_u=None, ld_v=None, ld_a=None, d_load=None, ld_load=None,
                                          damp_mass=0.0, damp_stiff=0.0):
        """lod_newmark_accel_direct with a column, two matrices and a factor per member; the factor is that of M."""
        self._check(self.lib.slod_lod_newmark_accel_ensemble_direct(
            self.h, _factor_ptr(factor), d_stiffness, n_members if ld_a_m is None else ld_a_m, d_mass,
            n_members if ld_m_m is None else ld_m_m, d_cols, damp_mass, damp_stiff, n_members, d_u,
            n_members if ld_u is None else ld_u, d_v, n_members if ld_v is None else ld_v, d_load,
            n_members if ld_load is None else ld_load, d_a, n_members if ld_a is None else ld_a))

    def lod_newmark_steps_ensemble_direct(self, factor, d_stiffness, d_mass, d_cols, dt, n_steps, n_members, d_u, d_v, d_a,
                                          beta=0.25, gamma=0.5, ld_a_m=None, ld_m_m=None, ld_u=None, ld_v=None, ld_a=None,
                                          d_load=None, ld_load=None, load_step_stride=0, damp_mass=0.0, damp_stiff=0.0,
                                          energies=True):
        """lod_newmark_steps_direct with a column, two matrices and a factor per member; the factor is that of
        lod_matrix_combine_ensemble(1 + gamma dt damp_mass, M, beta dt^2 + gamma dt damp_stiff, A).  Returns
        (kinetic, potential) as arrays [n_steps + 1, n_members], or (None, None) with energies=False."""
        shape = (max(n_steps, 0) + 1, max(n_members, 1))
        kin, pot = (np.zeros(shape), np.zeros(shape)) if energies else (None, None)
        self._check(self.lib.slod_lod_newmark_steps_ensemble_direct(
            self.h, _factor_ptr(factor), d_stiffness, n_members if ld_a_m is None else ld_a_m, d_mass,
            n_members if ld_m_m is None else ld_m_m, d_cols, dt, beta, gamma, damp_mass, damp_stiff, n_steps, n_members,
            d_u, n_members if ld_u is None else ld_u, d_v, n_members if ld_v is None else ld_v, d_a,
            n_members if ld_a is None else ld_a, d_load, n_members if ld_load is None else ld_load, load_step_stride,
            _dp(kin) if energies else None, _dp(pot) if energies else None))
        return kin, pot

    # ---- eigenpairs on a factor of S = A - sigma M, for one pencil and per ensemble member ----
    def lod_eigs_direct(self, factor, d_stiffness, d_mass, d_cols, n_eig, d_x, n_block=None, ld_x=None, start=0, tol=1e-10,
                        max_outer=200):
        """lod_eigs with the inner CG replaced by the factor of S = sym(A) - sigma M, sigma < lambda_1
        (lod_matrix_combine(1, A, -sigma, M)).  Returns (eigenvalues[n_block], residuals[n_block], outer iterations)."""
        if n_block is None:
            n_block = min(64, self.num_patches * self.spacedim, n_eig + max(4, n_eig // 2))
        lam = np.zeros(max(n_block, 1))
        res = np.zeros(max(n_block, 1))
        rc = self.lib.slod_lod_eigs_direct(self.h, _factor_ptr(factor), d_stiffness, d_mass, d_cols, n_eig, n_block, start, d_x,
                                           n_block if ld_x is None else ld_x, tol, max_outer, _dp(lam), _dp(res))
        if rc < 0:
            self._check(rc)
        return lam[:n_block], res[:n_block], rc

    def lod_eigs_ensemble_direct(self, factor, d_stiffness, d_mass, d_cols, n_members, n_eig, d_x, n_block=None, ld_a_m=None,
                                 ld_m_m=None, ld_x=None, start=0, tol=1e-10, max_outer=200, check=True):
        """lod_eigs_direct for the pencils of an ensemble: member k owns columns k * n_block .. of d_x, its matrices are member
        k of the ensemble matrices and its factor member k of `factor`.  Returns (eigenvalues[n_members, n_block],
        residuals[n_members, n_block], member_status[n_members], rc); member_status[k] is the outer iterations of member k
        or -5.  check=False: a failed member (rc = -5) does not raise."""
        if n_block is None:
            n_block = min(64, self.num_patches * self.spacedim, n_eig + max(4, n_eig // 2))
        shape = (max(n_members, 1), max(n_block, 1))
        lam, res = np.zeros(shape), np.zeros(shape)
        status = np.zeros(shape[0], dtype=np.intc)
        rc = self.lib.slod_lod_eigs_ensemble_direct(
            self.h, _factor_ptr(factor), d_stiffness, n_members if ld_a_m is None else ld_a_m, d_mass,
            n_members if ld_m_m is None else ld_m_m, d_cols, n_members, n_eig, n_block, start, d_x,
            n_members * n_block if ld_x is None else ld_x, tol, max_outer, _dp(lam), _dp(res),
            status.ctypes.data_as(C.POINTER(C.c_int)))
        if rc < 0 and (check or rc != -5):
            self._check(rc)
        return lam, res, status, rc

    # ---- eigenpairs nearest a shift sigma, on a factor of S = sym(A) - sigma M (LDL^T for an interior sigma) ----
    def lod_eigs_shift_direct(self, factor, sigma, d_stiffness, d_mass, d_cols, n_eig, d_x, n_block=None, ld_x=None, start=0,
                              tol=1e-10, max_outer=200):
        """lod_eigs_direct with the Ritz pairs ordered by their distance from sigma: the first n_eig columns are the pairs
        nearest sigma.  start=0 writes the hashed block of include/slod.h.  Returns (eigenvalues[n_block],
        residuals[n_block], outer iterations)."""
        if n_block is None:
            n_block = min(64, self.num_patches * self.spacedim, n_eig + max(4, n_eig // 2))
        lam = np.zeros(max(n_block, 1))
        res = np.zeros(max(n_block, 1))
        rc = self.lib.slod_lod_eigs_shift_direct(self.h, _factor_ptr(factor), sigma, d_stiffness, d_mass, d_cols, n_eig, n_block,
                                                 start, d_x, n_block if ld_x is None else ld_x, tol, max_outer, _dp(lam), _dp(res))
        if rc < 0:
            self._check(rc)
        return lam[:n_block], res[:n_block], rc

    def lod_eigs_shift_ensemble_direct(self, factor, sigma, d_stiffness, d_mass, d_cols, n_members, n_eig, d_x, n_block=None,
                                       ld_a_m=None, ld_m_m=None, ld_x=None, start=0, tol=1e-10, max_outer=200, check=True):
        """lod_eigs_shift_direct for the pencils of an ensemble, one sigma for all members; layout and returns of
        lod_eigs_ensemble_direct."""
        if n_block is None:
            n_block = min(64, self.num_patches * self.spacedim, n_eig + max(4, n_eig // 2))
        shape = (max(n_members, 1), max(n_block, 1))
        lam, res = np.zeros(shape), np.zeros(shape)
        status = np.zeros(shape[0], dtype=np.intc)
        rc = self.lib.slod_lod_eigs_shift_ensemble_direct(
            self.h, _factor_ptr(factor), sigma, d_stiffness, n_members if ld_a_m is None else ld_a_m, d_mass,
            n_members if ld_m_m is None else ld_m_m, d_cols, n_members, n_eig, n_block, start, d_x,
            n_members * n_block if ld_x is None else ld_x, tol, max_outer, _dp(lam), _dp(res),
            status.ctypes.data_as(C.POINTER(C.c_int)))
        if rc < 0 and (check or rc != -5):
            self._check(rc)
        return lam, res, status, rc

    def fem_rhs(self, d_f_qp, d_fine_rhs, stream=None):
        """Fine FEM load vector (d_f_qp = None: f = 1)."""
        self._check(self.lib.slod_fem_rhs(self.h, d_f_qp, d_fine_rhs, stream))

    def fem_solve(self, d_fine_rhs, d_fine_u, rel_tol=1e-12, max_iterations=20000, problem=0):
        res = C.c_double()
        it = self.lib.slod_fem_solve(self.h, problem, d_fine_rhs, d_fine_u, rel_tol, max_iterations, C.byref(res))
        if it < 0:
            self._check(it)
        return it, res.value

    # ---- coarse FEM(H) reference problem: Q1 on the N x N coarse mesh (raw device pointers as ints) ----
    def coarse_coefficient(self, field, d_out, problem=0, stream=None):
        """Coefficient `field` at the 2 x 2 Gauss points of every coarse cell, d_out [N][N][4]."""
        self._check(self.lib.slod_coarse_coefficient(self.h, problem, field, d_out, stream))

    def coarse_fem_rhs(self, d_f_cqp, d_coarse_rhs, stream=None):
        """Coarse FEM load vector [(N+1)^2][s] (d_f_cqp = None: f = 1)."""
        self._check(self.lib.slod_coarse_fem_rhs(self.h, d_f_cqp, d_coarse_rhs, stream))

    def coarse_fem_solve(self, d_coarse_rhs, d_coarse_u, rel_tol=1e-13, max_iterations=20000, problem=0):
        res = C.c_double()
        it = self.lib.slod_coarse_fem_solve(self.h, problem, d_coarse_rhs, d_coarse_u, rel_tol, max_iterations,
                                            C.byref(res))
        if it < 0:
            self._check(it)
        return it, res.value

    def coarse_interpolate(self, d_coarse, d_fine, stream=None):
        """Bilinear interpolation of a coarse nodal field [(N+1)^2][s] onto the fine grid [(NE+1)^2][s]."""
        self._check(self.lib.slod_coarse_interpolate(self.h, d_coarse, d_fine, stream))

    def error_norms(self, d_u, d_v=None, d_exact=None, d_exact_grad=None, problem=0, stream=None):
        """Norms of e = u - v - w on the fine grid (slod_compute_error_norms; raw device pointers, None = 0).
        Per-component lists and, as ParsedConvergenceTable groups components of one name, totals over the
        components: l2 and h1_semi in squares, h1 = (l2^2 + h1_semi^2)^{1/2} (deal.II's H1_norm), linf the
        maximum; energy = a(e,e)^{1/2} with the coefficient of `problem`.  Synchronises `stream`."""
        n = ErrorNorms()
        self._check(self.lib.slod_compute_error_norms(self.h, problem, d_u, d_v, d_exact, d_exact_grad, C.byref(n),
                                                      stream))
        s = self.spacedim
        l2 = [n.l2[c] for c in range(s)]
        h1s = [n.h1_semi[c] for c in range(s)]
        linf = [n.linf[c] for c in range(s)]
        l2t = float(np.sqrt(sum(x * x for x in l2)))
        h1st = float(np.sqrt(sum(x * x for x in h1s)))
        return {"l2_components": l2, "h1_semi_components": h1s, "linf_components": linf,
                "l2": l2t, "h1_semi": h1st, "h1": float(np.hypot(l2t, h1st)), "linf": max(linf),
                "energy": n.energy}

    def device_patch_layout(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        out = (PatchInfo * max(len(ids), 1))()
        self._check(self.lib.slod_device_patch_layout(self.h, ids.ctypes.data_as(C.POINTER(C.c_uint32)), len(ids), out))
        return [out[i] for i in range(len(ids))]

    def sample_coefficient(self, field, d_vals, r, problem=0):
        self._check(self.lib.slod_sample_coefficient(self.h, problem, field, d_vals, r))

    def compute_basis(self, gids, offsets=None, total=None):
        """Host-buffer path (slod_compute_basis). Returns (basis, premult) flat arrays."""
        gids = np.ascontiguousarray(gids, dtype=np.uint32)
        s = self.spacedim
        if offsets is None:
            sizes = [s * self.patch_layout(int(g) % self.num_patches).n_fine for g in gids]
            offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64) if len(gids) else \
                np.zeros(0, np.uint64)
            total = int(np.sum(sizes))
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        basis = np.zeros(total)
        premult = np.zeros(total)
        self._check(self.lib.slod_compute_basis(
            self.h, gids.ctypes.data_as(C.POINTER(C.c_uint32)), len(gids), _dp(basis), _dp(premult),
            offsets.ctypes.data_as(C.POINTER(C.c_uint64))))
        return basis, premult, offsets

    def assemble_stiffness_for_patch(self, gid):
        info = self.patch_layout(gid % self.num_patches)
        s = self.spacedim
        st = np.zeros((info.n_fine // s, 9, s, s))
        self._check(self.lib.slod_assemble_stiffness_for_patch(self.h, gid, _dp(st)))
        return st

    def patch_solution(self, gid):
        info = self.patch_layout(gid % self.num_patches)
        X = np.zeros((info.n_fine, info.n_coarse))
        self._check(self.lib.slod_patch_solution(self.h, gid, _dp(X)))
        return X
