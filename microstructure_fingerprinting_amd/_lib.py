"""ctypes binding of the C-ABI shared library ``libmfx.so`` (include/mfx.h).

The library is the product's only compute path.  If it is missing or no MI355X is
visible, calls raise -- there is no NumPy/CPU fallback.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmfx.so")

MFX_OK, MFX_ERR_ARG, MFX_ERR_G_RANGE, MFX_ERR_NO_DEVICE, MFX_ERR_HIP, MFX_ERR_UNSUPPORTED, MFX_ERR_DIR_NORM = range(7)

_lib = None

# every symbol include/mfx.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "mfx_last_error", "mfx_device_count", "mfx_abi_version",
    "mfx_tables_create", "mfx_tables_destroy", "mfx_tables_num_atoms",
    "mfx_plan_create_multishell", "mfx_plan_create_explicit", "mfx_plan_destroy", "mfx_plan_status",
    "mfx_rotate", "mfx_rotate_dev", "mfx_rotate_cols", "mfx_rotate_cols_dev", "mfx_fit_batch", "mfx_fit_batch_rows", "mfx_fit_batch_volume", "mfx_volume_rows", "mfx_thread_release", "mfx_fit_batch_dev",
    "mfx_solve_exhaustive", "mfx_monte_carlo_average", "mfx_monte_carlo_average_dev", "mfx_cleanup_2fascicles", "mfx_cleanup_2fascicles_dev", "mfx_last_kernel_ms", "mfx_set_profiling", "mfx_debug_set_stamps", "mfx_debug_last_fallback_count", "mfx_debug_last_guard_count", "mfx_debug_last_counter", "mfx_debug_set_k2_screen", "mfx_debug_set_k2_wide", "mfx_debug_set_k2x_screen", "mfx_debug_set_k2_maxc", "mfx_debug_set_k2x_maxc", "mfx_debug_set_k2s_cap", "mfx_debug_set_k2s_images", "mfx_debug_set_k3_cap", "mfx_debug_set_force_generic", "mfx_debug_set_k3_screen",
    "mfx_debug_seam",
]

# every symbol include/mfx_mcf.h declares (MCF signal synthesis; versioned on its own)
MCF_EXPORTS = ["mfx_mcf_abi_version", "mfx_mcf_pgse", "mfx_mcf_dde"]

# every symbol include/mfx_rot2d.h declares (2-D protocol rotation; versioned on its own)
ROT2D_EXPORTS = ["mfx_rot2d_abi_version", "mfx_rot2d_create", "mfx_rot2d_destroy", "mfx_rot2d_rotate",
                 "mfx_rot2d_rotate_dev", "mfx_rot2d_rotate_cols", "mfx_rot2d_rotate_cols_dev"]

# every symbol include/mfx_fit2d.h declares (batched fit of 2-D protocols; versioned on its own)
FIT2D_EXPORTS = ["mfx_fit2d_abi_version", "mfx_fit2d_max_atoms", "mfx_fit2d_batch_dev", "mfx_fit2d_batch",
                 "mfx_fit2d_debug_set_force_explicit"]

# every symbol include/mfx_wfit.h declares (weighted fit: per-voxel measurement weights; versioned on its own)
WFIT_EXPORTS = ["mfx_wfit_abi_version", "mfx_wfit_max_atoms", "mfx_wfit_batch_dev", "mfx_wfit_batch",
                "mfx_wfit_debug_set_force_explicit"]

# every symbol include/mfx_predict.h declares (forward model and magnitude noise; versioned on its own)
PREDICT_EXPORTS = ["mfx_predict_abi_version", "mfx_predict_dev", "mfx_predict", "mfx_sos_noise_dev", "mfx_sos_noise"]

# every symbol include/mfx_profile.h declares (objective profiles; versioned on its own)
PROFILE_EXPORTS = ["mfx_profile_abi_version", "mfx_profile_cut", "mfx_profile_max_atoms", "mfx_profile_dev", "mfx_profile",
                   "mfx_pair_objectives_dev", "mfx_pair_objectives", "mfx_profile_debug_last_config"]

# every symbol include/mfx_post.h declares (soft fits: posterior weights per atom; versioned on its own)
POST_EXPORTS = ["mfx_post_abi_version", "mfx_post_max_atoms", "mfx_post_dev", "mfx_post", "mfx_post_debug_last_config"]

# every symbol include/mfx_wsoft.h declares (profiles and soft fits of a weighted fit; versioned on its own)
WSOFT_EXPORTS = ["mfx_wsoft_abi_version", "mfx_wsoft_max_atoms", "mfx_wpost_dev", "mfx_wpost", "mfx_wprofile_dev", "mfx_wprofile",
                 "mfx_wpair_objectives_dev", "mfx_wpair_objectives"]

# every symbol include/mfx_soft2d.h declares (soft fits and objective profiles of 2-D protocols; versioned on its own)
SOFT2D_EXPORTS = ["mfx_soft2d_abi_version", "mfx_soft2d_max_atoms", "mfx_post2d_dev", "mfx_post2d", "mfx_profile2d_dev",
                  "mfx_profile2d"]

# every symbol include/mfx_w2d.h declares (measurement weights for 2-D protocols: fit, posterior, profile; versioned on its own)
W2D_EXPORTS = ["mfx_w2d_abi_version", "mfx_w2d_max_atoms", "mfx_wfit2d_batch_dev", "mfx_wfit2d_batch", "mfx_wpost2d_dev",
               "mfx_wpost2d", "mfx_wprofile2d_dev", "mfx_wprofile2d", "mfx_w2d_debug_set_force_explicit"]

# every symbol include/mfx_robust.h declares (robust fits: residual-driven reweighting on the device; versioned on its own)
ROBUST_EXPORTS = ["mfx_robust_abi_version", "mfx_robust_weights_dev", "mfx_rfit_batch_dev", "mfx_rfit_batch"]

# every symbol include/mfx_predict2d.h declares (forward model of 2-D protocols; versioned on its own)
PREDICT2D_EXPORTS = ["mfx_predict2d_abi_version", "mfx_predict2d_dev", "mfx_predict2d"]

# every symbol include/mfx_robust2d.h declares (robust fits of 2-D protocols; versioned on its own)
ROBUST2D_EXPORTS = ["mfx_robust2d_abi_version", "mfx_rfit2d_batch_dev", "mfx_rfit2d_batch",
                    "mfx_robust2d_debug_last_plan_directions"]

# every symbol include/mfx_boot.h declares (bootstrap: resampled refits reduced on the device; versioned on its own)
BOOT_EXPORTS = ["mfx_boot_abi_version", "mfx_boot_resample_dev", "mfx_boot_gather_dev", "mfx_boot_reduce_dev",
                "mfx_boot_fit_dev", "mfx_boot_fit"]

# every symbol include/mfx_boot2d.h declares (bootstrap of 2-D protocols, fits shared per voxel; versioned on its own)
BOOT2D_EXPORTS = ["mfx_boot2d_abi_version", "mfx_boot2d_rep_tile", "mfx_boot2d_debug_set_force_plain",
                  "mfx_boot2d_fit_rows_dev", "mfx_boot2d_fit_dev", "mfx_boot2d_fit"]

# every symbol include/mfx_wboot.h declares (bootstrap conditional on a fit's measurement weights; versioned on its own)
WBOOT_EXPORTS = ["mfx_wboot_abi_version", "mfx_wboot_rep_tile", "mfx_wboot_debug_set_force_plain", "mfx_wboot_resample_dev",
                 "mfx_wboot_fit_rows_dev", "mfx_wboot_fit_dev", "mfx_wboot_fit"]

# every symbol include/mfx_wboot2d.h declares (bootstrap of 2-D protocols conditional on measurement weights; versioned on its own)
WBOOT2D_EXPORTS = ["mfx_wboot2d_abi_version", "mfx_wboot2d_rep_tile", "mfx_wboot2d_max_atoms", "mfx_wboot2d_debug_set_force_plain",
                   "mfx_wboot2d_fit_rows_dev", "mfx_wboot2d_fit_dev", "mfx_wboot2d_fit"]

# every symbol include/mfx_solve.h declares (batched explicit-dictionary solver: many signals, one dictionary; versioned on its own)
SOLVE_EXPORTS = ["mfx_solve_abi_version", "mfx_solve_create", "mfx_solve_destroy", "mfx_solve_num_columns",
                 "mfx_solve_bytes_per_signal", "mfx_solve_batch_dev", "mfx_solve_batch", "mfx_solve_debug_set_force_generic"]

# every symbol include/mfx_solve_soft.h declares (objective profiles and posteriors on a solver handle; versioned on its own)
SOLVE_SOFT_EXPORTS = ["mfx_solve_soft_abi_version", "mfx_solve_soft_served", "mfx_solve_soft_bytes_per_signal",
                      "mfx_solve_profile_dev", "mfx_solve_profile", "mfx_solve_post_dev", "mfx_solve_post"]
SOLVE_SOFT_PROFILE, SOLVE_SOFT_POST = 0, 1   # `what` of mfx_solve_soft_bytes_per_signal


class MfxError(RuntimeError):
    pass


def lib():
    """Load libmfx.so (fails loudly if the HIP extension has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MfxError("HIP extension %s not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(or `make -C microstructure_fingerprinting_amd/csrc`). There is no CPU fallback." % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    dp = C.POINTER(C.c_double)
    ip = C.POINTER(C.c_int32)
    lp = C.POINTER(C.c_int64)
    bp = C.POINTER(C.c_uint8)
    vp = C.c_void_p
    L.mfx_last_error.restype = C.c_char_p
    L.mfx_device_count.restype = C.c_int
    L.mfx_abi_version.restype = C.c_int
    L.mfx_tables_create.argtypes = [dp, ip, dp, dp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.mfx_tables_destroy.argtypes = [vp]
    L.mfx_tables_destroy.restype = None
    L.mfx_tables_num_atoms.argtypes = [vp]
    L.mfx_plan_create_multishell.argtypes = [vp, dp, C.c_int, C.POINTER(vp)]
    L.mfx_plan_create_explicit.argtypes = [vp, dp, ip, C.c_int, C.POINTER(vp)]
    L.mfx_plan_destroy.argtypes = [vp]
    L.mfx_plan_destroy.restype = None
    L.mfx_plan_status.argtypes = [vp, vp]
    L.mfx_rotate.argtypes = [vp, dp, C.c_int64, C.c_int, dp]
    L.mfx_rotate_dev.argtypes = [vp, vp, C.c_int64, C.c_int, vp, vp]
    L.mfx_rotate_cols.argtypes = [vp, dp, ip, C.c_int64, C.c_int, dp]
    L.mfx_rotate_cols_dev.argtypes = [vp, vp, vp, C.c_int64, C.c_int, vp, vp]
    L.mfx_fit_batch.argtypes = [vp, dp, ip, bp, bp, dp, C.c_int, C.c_int, C.c_int, dp, dp, C.c_int, C.c_int64, dp]
    L.mfx_fit_batch_rows.argtypes = [vp, dp, lp, ip, bp, bp, dp, C.c_int, C.c_int, C.c_int, dp, dp, C.c_int, C.c_int64, dp]
    L.mfx_fit_batch_volume.argtypes = [vp, vp, C.c_int, C.c_double, C.c_double, C.c_int64, lp, ip, bp, bp, dp, C.c_int, C.c_int,
                                       C.c_int, dp, dp, C.c_int, C.c_int64, dp]
    L.mfx_volume_rows.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_int64, C.c_int, lp, C.c_int64, dp, C.c_int]
    L.mfx_fit_batch_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int64, vp, vp]
    L.mfx_solve_exhaustive.argtypes = [dp, C.c_int64, C.c_int, lp, C.c_int, dp, dp, lp, lp, dp, dp]
    L.mfx_monte_carlo_average.argtypes = [dp, C.c_int64, C.c_int, lp, dp, C.c_double, C.c_int64, C.c_int64, dp, C.c_int]
    L.mfx_monte_carlo_average_dev.argtypes = [vp, C.c_int64, C.c_int64, C.c_int64, C.c_int, lp, dp, C.c_double, C.c_int64,
                                              C.c_int64, dp, vp]
    L.mfx_cleanup_2fascicles.argtypes = [dp, dp, dp, dp, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double, dp, dp, C.c_int]
    L.mfx_cleanup_2fascicles_dev.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double, vp, vp, vp]
    L.mfx_last_kernel_ms.restype = C.c_double
    L.mfx_set_profiling.argtypes = [C.c_int]
    L.mfx_set_profiling.restype = None
    L.mfx_debug_set_stamps.argtypes = [vp]
    L.mfx_debug_set_stamps.restype = None
    L.mfx_debug_last_fallback_count.restype = C.c_int
    L.mfx_debug_last_guard_count.restype = C.c_int
    L.mfx_debug_last_counter.argtypes = [C.c_int]
    L.mfx_debug_last_counter.restype = C.c_int
    L.mfx_debug_set_k2x_maxc.argtypes = [C.c_int]
    L.mfx_debug_set_k2x_maxc.restype = None
    L.mfx_debug_set_k2_screen.argtypes = [C.c_int]
    L.mfx_debug_set_k2_screen.restype = None
    L.mfx_debug_set_k2_wide.argtypes = [C.c_int]
    L.mfx_debug_set_k2_wide.restype = None
    L.mfx_debug_set_k2x_screen.argtypes = [C.c_int]
    L.mfx_debug_set_k2x_screen.restype = None
    L.mfx_debug_set_k2_maxc.argtypes = [C.c_int]
    L.mfx_debug_set_k2_maxc.restype = None
    L.mfx_debug_set_k2s_cap.argtypes = [C.c_int]
    L.mfx_debug_set_k2s_cap.restype = None
    L.mfx_debug_set_k3_cap.argtypes = [C.c_int]
    L.mfx_debug_set_k3_cap.restype = None
    L.mfx_debug_set_force_generic.argtypes = [C.c_int]
    L.mfx_debug_set_force_generic.restype = None
    L.mfx_debug_set_k3_screen.argtypes = [C.c_int]
    L.mfx_debug_set_k3_screen.restype = None
    L.mfx_debug_set_k2s_images.argtypes = [C.c_int]
    L.mfx_debug_set_k2s_images.restype = None
    L.mfx_debug_seam.argtypes = [C.c_int, C.c_int, C.c_int64]
    L.mfx_debug_seam.restype = C.c_int64
    L.mfx_mcf_abi_version.restype = C.c_int
    for fn in ("mfx_mcf_pgse", "mfx_mcf_dde"):
        getattr(L, fn).argtypes = [dp, dp, C.c_int, dp, C.c_int64, dp, dp, C.c_int64, dp, C.c_double, dp]
        getattr(L, fn).restype = C.c_int
    L.mfx_rot2d_abi_version.restype = C.c_int
    L.mfx_rot2d_create.argtypes = [dp, C.c_int, ip, ip, C.c_int, ip, dp, ip, ip, ip, dp, C.c_int, ip, dp, dp, C.c_int,
                                   C.c_int, C.c_double, C.c_double, C.c_int, C.POINTER(vp)]
    L.mfx_rot2d_destroy.argtypes = [vp]
    L.mfx_rot2d_destroy.restype = None
    L.mfx_rot2d_rotate.argtypes = [vp, dp, C.c_int64, dp, ip]
    L.mfx_rot2d_rotate_dev.argtypes = [vp, vp, C.c_int64, vp, vp, vp]
    L.mfx_rot2d_rotate_cols.argtypes = [vp, dp, ip, C.c_int64, dp, ip]
    L.mfx_rot2d_rotate_cols_dev.argtypes = [vp, vp, vp, C.c_int64, vp, vp, vp]
    L.mfx_fit2d_abi_version.restype = C.c_int
    L.mfx_fit2d_max_atoms.argtypes = [vp, C.c_int]
    L.mfx_fit2d_batch_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int64, vp, vp, vp]
    L.mfx_fit2d_batch.argtypes = [vp, dp, ip, bp, dp, C.c_int, C.c_int, dp, C.c_int64, dp, ip]
    L.mfx_fit2d_debug_set_force_explicit.argtypes = [C.c_int]
    L.mfx_fit2d_debug_set_force_explicit.restype = None
    L.mfx_wfit_abi_version.restype = C.c_int
    L.mfx_wfit_max_atoms.argtypes = [vp, C.c_int]
    L.mfx_wfit_batch_dev.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int, C.c_int64, vp, vp, vp]
    L.mfx_wfit_batch.argtypes = [vp, dp, dp, C.c_int64, ip, bp, dp, C.c_int, C.c_int, dp, C.c_int64, dp, ip]
    L.mfx_wfit_debug_set_force_explicit.argtypes = [C.c_int]
    L.mfx_wfit_debug_set_force_explicit.restype = None
    L.mfx_predict_abi_version.restype = C.c_int
    L.mfx_predict_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int64, vp, vp, C.c_int, C.c_int,
                                  C.c_uint64, C.c_uint64, vp, vp, vp, vp]
    L.mfx_predict.argtypes = [vp, dp, dp, C.c_int, C.c_int, C.c_int, dp, dp, C.c_int, C.c_int64, dp, dp, C.c_int, C.c_int,
                              C.c_uint64, C.c_uint64, dp, dp]
    L.mfx_sos_noise_dev.argtypes = [vp, C.c_int64, vp, C.c_int, C.c_int, C.c_uint64, C.c_uint64, vp, C.c_int, vp]
    L.mfx_sos_noise.argtypes = [dp, C.c_int64, dp, C.c_int, C.c_int, C.c_uint64, C.c_uint64, dp, C.c_int]
    L.mfx_profile_abi_version.restype = C.c_int
    L.mfx_profile_cut.restype = C.c_double
    L.mfx_profile_max_atoms.argtypes = [vp, C.c_int, C.c_int]
    L.mfx_profile_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.c_int64, vp, vp, vp]
    L.mfx_profile.argtypes = [vp, dp, dp, C.c_int, C.c_int, dp, C.c_int64, dp, ip]
    L.mfx_pair_objectives_dev.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int64, vp, vp]
    L.mfx_pair_objectives.argtypes = [vp, dp, dp, C.c_int, dp, C.c_int64, dp]
    L.mfx_profile_debug_last_config.argtypes = [ip]
    L.mfx_post_abi_version.restype = C.c_int
    L.mfx_post_max_atoms.argtypes = [vp, C.c_int]
    L.mfx_post_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int64, vp, vp, vp, vp]
    L.mfx_post.argtypes = [vp, dp, dp, C.c_int, C.c_int, dp, dp, dp, C.c_int64, dp, dp, ip]
    L.mfx_post_debug_last_config.argtypes = [ip]
    L.mfx_wsoft_abi_version.restype = C.c_int
    L.mfx_wsoft_max_atoms.argtypes = [vp, C.c_int, C.c_int]
    L.mfx_wpost_dev.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int64, vp, vp, vp, vp]
    L.mfx_wpost.argtypes = [vp, dp, dp, C.c_int64, dp, C.c_int, C.c_int, dp, dp, dp, C.c_int64, dp, dp, ip]
    L.mfx_wprofile_dev.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int, C.c_int, vp, C.c_int64, vp, vp, vp]
    L.mfx_wprofile.argtypes = [vp, dp, dp, C.c_int64, dp, C.c_int, C.c_int, dp, C.c_int64, dp, ip]
    L.mfx_wpair_objectives_dev.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int, vp, C.c_int64, vp, vp]
    L.mfx_wpair_objectives.argtypes = [vp, dp, dp, C.c_int64, dp, C.c_int, dp, C.c_int64, dp]
    L.mfx_soft2d_abi_version.restype = C.c_int
    L.mfx_soft2d_max_atoms.argtypes = [vp, C.c_int]
    L.mfx_post2d_dev.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int64, vp, vp, vp, vp, vp]
    L.mfx_post2d.argtypes = [vp, dp, dp, C.c_int, dp, dp, C.c_int64, dp, dp, ip, ip]
    L.mfx_profile2d_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int64, vp, vp, vp, vp]
    L.mfx_profile2d.argtypes = [vp, dp, dp, C.c_int, C.c_int64, dp, ip, ip]
    L.mfx_w2d_abi_version.restype = C.c_int
    L.mfx_w2d_max_atoms.argtypes = [vp, C.c_int]
    L.mfx_wfit2d_batch_dev.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int, C.c_int64, vp, vp, vp, vp]
    L.mfx_wfit2d_batch.argtypes = [vp, dp, dp, C.c_int64, ip, bp, dp, C.c_int, C.c_int, dp, C.c_int64, dp, ip, ip]
    L.mfx_wpost2d_dev.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int, vp, vp, C.c_int64, vp, vp, vp, vp, vp]
    L.mfx_wpost2d.argtypes = [vp, dp, dp, C.c_int64, dp, C.c_int, dp, dp, C.c_int64, dp, dp, ip, ip]
    L.mfx_wprofile2d_dev.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int, C.c_int64, vp, vp, vp, vp]
    L.mfx_wprofile2d.argtypes = [vp, dp, dp, C.c_int64, dp, C.c_int, C.c_int64, dp, ip, ip]
    L.mfx_w2d_debug_set_force_explicit.argtypes = [C.c_int]
    L.mfx_w2d_debug_set_force_explicit.restype = None
    L.mfx_robust_abi_version.restype = C.c_int
    L.mfx_robust_weights_dev.argtypes = [C.c_int, vp, vp, vp, C.c_int64, C.c_int, C.c_double, C.c_int64, vp, vp, vp, vp, vp, vp]
    L.mfx_rfit_batch_dev.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int64, vp, vp, vp, vp,
                                     vp, vp, vp]
    L.mfx_rfit_batch.argtypes = [vp, dp, dp, C.c_int64, ip, bp, dp, C.c_int, C.c_int, dp, C.c_int, C.c_double, C.c_int, C.c_int64,
                                 dp, dp, dp, ip, ip, lp, ip]
    L.mfx_predict2d_abi_version.restype = C.c_int
    L.mfx_predict2d_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.c_int64, vp, vp, C.c_int, C.c_int, C.c_uint64, C.c_uint64,
                                    vp, vp, vp, vp, vp]
    L.mfx_predict2d.argtypes = [vp, dp, dp, C.c_int, C.c_int, dp, C.c_int64, dp, dp, C.c_int, C.c_int, C.c_uint64, C.c_uint64,
                                dp, dp, ip]
    L.mfx_robust2d_abi_version.restype = C.c_int
    L.mfx_rfit2d_batch_dev.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int64, vp, vp, vp, vp,
                                       vp, vp, vp, vp]
    L.mfx_rfit2d_batch.argtypes = [vp, dp, dp, C.c_int64, ip, bp, dp, C.c_int, C.c_int, dp, C.c_int, C.c_double, C.c_int, C.c_int64,
                                   dp, dp, dp, ip, ip, ip, lp, ip]
    L.mfx_robust2d_debug_last_plan_directions.restype = C.c_int64
    L.mfx_boot_abi_version.restype = C.c_int
    L.mfx_boot_resample_dev.argtypes = [C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int64, C.c_int, C.c_int,
                                        C.c_int, C.c_uint64, C.c_uint64, vp, vp, vp, vp]
    L.mfx_boot_gather_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int64, C.c_int, vp, vp, vp, vp]
    L.mfx_boot_reduce_dev.argtypes = [vp, vp, C.c_int64, C.c_int, C.c_int, vp, C.c_int, vp, vp]
    L.mfx_boot_fit_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int64, C.c_int,
                                   C.c_int, C.c_int, C.c_uint64, C.c_uint64, vp, C.c_int, vp, C.c_int, C.c_int64, vp, vp, vp, vp, vp]
    L.mfx_boot_fit.argtypes = [vp, dp, ip, bp, bp, dp, C.c_int, C.c_int, C.c_int, dp, dp, C.c_int, dp, ip, lp, C.c_int64, C.c_int,
                               C.c_int, C.c_int, C.c_uint64, C.c_uint64, dp, C.c_int, dp, C.c_int, C.c_int64, dp, ip, ip, dp]
    L.mfx_boot2d_abi_version.restype = C.c_int
    L.mfx_boot2d_rep_tile.restype = C.c_int
    L.mfx_boot2d_debug_set_force_plain.argtypes = [C.c_int]
    L.mfx_boot2d_debug_set_force_plain.restype = None
    L.mfx_boot2d_fit_rows_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int64, C.c_int, vp, vp, vp]
    L.mfx_boot2d_fit_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int64, C.c_int, C.c_int, C.c_int,
                                     C.c_uint64, C.c_uint64, vp, C.c_int, vp, C.c_int, C.c_int64, vp, vp, vp, vp, vp, vp]
    L.mfx_boot2d_fit.argtypes = [vp, dp, ip, bp, dp, C.c_int, C.c_int, dp, dp, ip, lp, C.c_int64, C.c_int, C.c_int, C.c_int,
                                 C.c_uint64, C.c_uint64, dp, C.c_int, dp, C.c_int, C.c_int64, dp, ip, ip, ip, dp]
    L.mfx_wboot_abi_version.restype = C.c_int
    L.mfx_wboot_rep_tile.restype = C.c_int
    L.mfx_wboot_debug_set_force_plain.argtypes = [C.c_int]
    L.mfx_wboot_debug_set_force_plain.restype = None
    L.mfx_wboot_resample_dev.argtypes = [C.c_int, vp, vp, vp, C.c_int64, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int64, C.c_int,
                                         C.c_int, C.c_int, C.c_uint64, C.c_uint64, vp, vp, vp, vp]
    L.mfx_wboot_fit_rows_dev.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int, C.c_int64, C.c_int, vp, vp, vp]
    L.mfx_wboot_fit_dev.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int64, C.c_int, C.c_int,
                                    C.c_int, C.c_uint64, C.c_uint64, vp, C.c_int, vp, C.c_int, C.c_int64, vp, vp, vp, vp, vp]
    L.mfx_wboot_fit.argtypes = [vp, dp, dp, C.c_int64, ip, bp, dp, C.c_int, C.c_int, dp, dp, ip, lp, C.c_int64, C.c_int, C.c_int,
                                C.c_int, C.c_uint64, C.c_uint64, dp, C.c_int, dp, C.c_int, C.c_int64, dp, ip, ip, dp]
    L.mfx_wboot2d_abi_version.restype = C.c_int
    L.mfx_wboot2d_rep_tile.restype = C.c_int
    L.mfx_wboot2d_max_atoms.argtypes = [vp]
    L.mfx_wboot2d_max_atoms.restype = C.c_int
    L.mfx_wboot2d_debug_set_force_plain.argtypes = [C.c_int]
    L.mfx_wboot2d_debug_set_force_plain.restype = None
    L.mfx_wboot2d_fit_rows_dev.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int, C.c_int64, C.c_int, vp, vp, vp, vp]
    L.mfx_wboot2d_fit_dev.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int64, C.c_int, C.c_int,
                                      C.c_int, C.c_uint64, C.c_uint64, vp, C.c_int, vp, C.c_int, C.c_int64, vp, vp, vp, vp, vp, vp]
    L.mfx_wboot2d_fit.argtypes = [vp, dp, dp, C.c_int64, ip, bp, dp, C.c_int, C.c_int, dp, dp, ip, lp, C.c_int64, C.c_int, C.c_int,
                                  C.c_int, C.c_uint64, C.c_uint64, dp, C.c_int, dp, C.c_int, C.c_int64, dp, ip, ip, ip, dp]
    L.mfx_solve_abi_version.restype = C.c_int
    L.mfx_solve_create.argtypes = [dp, C.c_int64, C.c_int, lp, C.c_int, C.c_int, C.POINTER(vp)]
    L.mfx_solve_destroy.argtypes = [vp]
    L.mfx_solve_destroy.restype = None
    L.mfx_solve_num_columns.argtypes = [vp]
    L.mfx_solve_num_columns.restype = C.c_int64
    L.mfx_solve_bytes_per_signal.argtypes = [vp]
    L.mfx_solve_bytes_per_signal.restype = C.c_int64
    L.mfx_solve_batch_dev.argtypes = [vp, vp, C.c_int64, C.c_int64, vp, vp, vp, vp, vp, vp]
    L.mfx_solve_batch.argtypes = [vp, dp, C.c_int64, C.c_int64, dp, lp, dp, dp, ip]
    L.mfx_solve_debug_set_force_generic.argtypes = [C.c_int]
    L.mfx_solve_debug_set_force_generic.restype = None
    L.mfx_solve_soft_abi_version.restype = C.c_int
    L.mfx_solve_soft_served.argtypes = [vp]
    L.mfx_solve_soft_bytes_per_signal.argtypes = [vp, C.c_int]
    L.mfx_solve_soft_bytes_per_signal.restype = C.c_int64
    L.mfx_solve_profile_dev.argtypes = [vp, vp, C.c_int64, C.c_int64, vp, vp, vp, vp, vp, vp]
    L.mfx_solve_profile.argtypes = [vp, dp, C.c_int64, C.c_int64, dp, dp, ip, ip, ip]
    L.mfx_solve_post_dev.argtypes = [vp, vp, C.c_int64, vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp]
    L.mfx_solve_post.argtypes = [vp, dp, C.c_int64, dp, dp, C.c_int64, dp, dp, dp, dp, ip]
    _lib = L
    return L


def check(rc):
    """Map a C status code to the exception class the reference raises for that condition."""
    if rc == MFX_OK:
        return
    msg = lib().mfx_last_error().decode("utf-8", "replace")
    if rc in (MFX_ERR_G_RANGE, MFX_ERR_DIR_NORM):
        raise ValueError(msg)             # mf_utils.py:1798-1802, 1829-1836
    if rc == MFX_ERR_ARG:
        raise ValueError(msg)
    if rc == MFX_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise MfxError(msg)


def dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def lptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def bptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def opt(a, ptr=dptr):
    """The pointer of an optional array: ``ptr(a)``, or None (a null pointer) without one."""
    return ptr(a) if a is not None else None


def f64c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def f64c_opt(a):
    return np.ascontiguousarray(a, dtype=np.float64) if a is not None else None
