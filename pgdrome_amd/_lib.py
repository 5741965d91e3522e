"""ctypes binding of include/pgd_amd.h (libpgd_amd.so).

This is the whole Python <-> native boundary: plain pointers, sizes and 64-bit
handles.  Loading never falls back to a CPU implementation: a missing library
or a missing GPU raises.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

LIB_PATH = Path(__file__).resolve().parent / "lib" / "libpgd_amd.so"

H = C.c_int64
I64 = C.c_int64
I32 = C.c_int32
F64 = C.c_double
PD = C.POINTER(C.c_double)
PI32 = C.POINTER(C.c_int32)
PI64 = C.POINTER(C.c_int64)
PH = C.POINTER(C.c_int64)
VP = C.c_void_p

PU8 = C.POINTER(C.c_uint8)
HALO_FN = C.CFUNCTYPE(C.c_int, VP, H, I64, I64, I64, I64)      # pgd_halo_fn
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, VP, C.c_int, C.c_int)      # pgd_allreduce_fn

# name -> (restype, argtypes); mirrors include/pgd_amd.h declaration by declaration
SIGNATURES = {
    "pgd_ctx_create": (C.c_int, [C.c_int, VP, PH]),
    "pgd_ctx_destroy": (C.c_int, [H]),
    "pgd_sync": (C.c_int, [H]),
    "pgd_last_error": (C.c_char_p, [H]),
    "pgd_version": (C.c_int, []),
    "pgd_device_count": (C.c_int, []),
    "pgd_mesh_upload": (C.c_int, [H, PD, I64, C.c_int, PI32, I64, C.c_int, PH]),
    "pgd_mesh_blocked": (C.c_int, [H, H, C.c_int, PH]),
    "pgd_mesh_p2_bind": (C.c_int, [H, H, H, PI32, I64, C.POINTER(C.c_int)]),
    "pgd_atom_embed": (C.c_int, [H, H, H, C.c_int, C.c_int, F64, H, PH]),
    "pgd_mesh_info": (C.c_int, [H, H, PI64, PI64, PI64, PI32, PI32, PI32]),
    "pgd_mesh_pattern_download": (C.c_int, [H, H, PI32, PI32]),
    "pgd_mesh_sym_info": (C.c_int, [H, H, PI32, PI32, PI32]),
    "pgd_mesh_dict_count": (C.c_int, [H, H, PI32]),
    "pgd_mesh_lattice": (C.c_int, [H, H, PI32, PD]),
    "pgd_mesh_free": (C.c_int, [H, H]),
    "pgd_vec_alloc": (C.c_int, [H, I64, PH]),
    "pgd_vec_free": (C.c_int, [H, H]),
    "pgd_vec_size": (C.c_int, [H, H, PI64]),
    "pgd_vec_upload": (C.c_int, [H, H, PD, I64, I64]),
    "pgd_vec_download": (C.c_int, [H, H, PD, I64, I64]),
    "pgd_vec_ptr": (C.c_int, [H, H, C.POINTER(VP)]),
    "pgd_vec_fill": (C.c_int, [H, H, F64]),
    "pgd_vec_copy": (C.c_int, [H, H, H]),
    "pgd_vec_copy_range": (C.c_int, [H, H, I64, H, I64, I64]),
    "pgd_vec_scale": (C.c_int, [H, H, F64]),
    "pgd_vec_mul": (C.c_int, [H, H, H, H]),
    "pgd_vec_axpy": (C.c_int, [H, H, F64, H]),
    "pgd_vec_set": (C.c_int, [H, H, PI32, PD, I64]),
    "pgd_vec_lincomb": (C.c_int, [H, H, PH, PD, C.c_int]),
    "pgd_vec_lincomb_inplace": (C.c_int, [H, H, PH, PD, C.c_int]),
    "pgd_vec_dot": (C.c_int, [H, H, H, I64, I64, PD]),
    "pgd_block_create": (C.c_int, [H, I64, C.c_int, C.c_int, PH]),
    "pgd_block_free": (C.c_int, [H, H]),
    "pgd_block_info": (C.c_int, [H, H, PI64, C.POINTER(C.c_int), C.POINTER(C.c_int), PI64]),
    "pgd_block_storage": (C.c_int, [H, C.POINTER(C.c_int)]),
    "pgd_block_set_column": (C.c_int, [H, H, C.c_int, H]),
    "pgd_block_get_column": (C.c_int, [H, H, C.c_int, H]),
    "pgd_block_dots": (C.c_int, [H, H, H, I64, I64, PD]),
    "pgd_block_combine": (C.c_int, [H, H, PD, H, H]),
    "pgd_eval_batch": (C.c_int, [H, PH, C.c_int, PD, I64, C.c_int, F64, PD, H, H, H, H]),
    "pgd_eval_batch_norm": (C.c_int, [H, PH, C.c_int, C.c_int, PD, I64, C.c_int, F64, PD, H, H, H, H]),
    "pgd_cell_gradient": (C.c_int, [H, H, H, PD, C.c_int, H, H]),
    "pgd_eval_batch_grad": (C.c_int, [H, H, PH, C.c_int, PD, C.c_int, H, PD, I64, C.c_int, F64, PD, H, H, H, H]),
    "pgd_eval_norm_last_shape": (C.c_int, [H, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pgd_cell_gradient_p2": (C.c_int, [H, H, H, PD, C.c_int, PD, C.c_int, H, H]),
    "pgd_eval_batch_grad_p2": (C.c_int, [H, H, PH, C.c_int, PD, C.c_int, PD, C.c_int, H, PD, I64, C.c_int, F64, PD, H, H, H, H]),
    "pgd_eval_batch_quantity": (C.c_int, [H, PH, C.c_int, C.c_int, C.c_int, PD, I64, C.c_int, F64, PD, H, H, H, H]),
    "pgd_eval_batch_grad_quantity": (C.c_int, [H, H, PH, C.c_int, PD, C.c_int, C.c_int, H, PD, I64, C.c_int, F64, PD, H, H, H, H]),
    "pgd_eval_batch_grad_p2_quantity": (C.c_int, [H, H, PH, C.c_int, PD, C.c_int, PD, C.c_int, C.c_int, H, PD, I64, C.c_int, F64, PD, H, H, H,
                                                  H]),
    "pgd_atom_assemble": (C.c_int, [H, H, C.c_int, C.c_int, C.c_int, H, PH]),
    "pgd_atom_assemble_cells": (C.c_int, [H, H, C.c_int, C.c_int, C.c_int, H, PU8, I64, PH]),
    "pgd_atom_assemble_cellwise": (C.c_int, [H, H, C.c_int, C.c_int, C.c_int, H, H, PU8, I64, PH]),
    "pgd_atom_assemble_facets": (C.c_int, [H, H, PI32, I64, C.c_int, PH]),
    "pgd_atom_upload": (C.c_int, [H, H, PD, PH]),
    "pgd_atom_download": (C.c_int, [H, H, PD]),
    "pgd_atom_free": (C.c_int, [H, H]),
    "pgd_op_combine": (C.c_int, [H, H, PH, PD, C.c_int, PI32, I64, PH]),
    "pgd_spmv": (C.c_int, [H, H, H, H, I64, I64]),
    "pgd_bilinear": (C.c_int, [H, H, H, H, I64, I64, PD]),
    "pgd_bilinear_many": (C.c_int, [H, H, H, PH, C.c_int, I64, I64, PD]),
    "pgd_start_gram": (C.c_int, [H, H, PH, C.c_int, H, I64, I64, PD]),
    "pgd_start_residual": (C.c_int, [H, H, C.c_int, PD, H, H]),
    "pgd_mg_slab_setup": (C.c_int, [H, H, C.c_int, C.c_int, I64, I64, C.POINTER(I64), C.POINTER(C.c_int)]),
    "pgd_mg_slab_fix_start": (C.c_int, [H, H, H, H, I64, I64]),
    "pgd_mg_slab_down": (C.c_int, [H, H, H]),
    "pgd_mg_slab_restrict": (C.c_int, [H, H, H]),
    "pgd_mg_coarse": (C.c_int, [H, H, H]),
    "pgd_mg_slab_up": (C.c_int, [H, H, H, H, H, C.c_int, PD]),
    "pgd_bicgstab_solve": (C.c_int, [H, H, H, H, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_int), PD]),
    "pgd_atom_product_form": (C.c_int, [H, H, C.POINTER(C.c_int)]),
    "pgd_product_plan": (C.c_int, [H, H, I64, I64, C.c_int, PI64, C.c_int]),
    "pgd_vec_multidot": (C.c_int, [H, H, PH, C.c_int, I64, I64, PD]),
    "pgd_vec_multidot_pair": (C.c_int, [H, H, H, PH, C.c_int, I64, I64, PD]),
    "pgd_vec_gram": (C.c_int, [H, PH, C.c_int, PH, C.c_int, I64, I64, PD]),
    "pgd_quad_forms": (C.c_int, [H, PH, C.c_int, PD, C.c_int, C.c_int, PH, PD]),
    "pgd_grid_misfit": (C.c_int, [H, PD, PD, C.c_int, C.c_int, PD, PI32, C.c_int, H, PD, PI64]),
    "pgd_grid_posterior": (C.c_int, [H, H, F64, PD, PI32, C.c_int, C.c_int, PD, PD, C.c_int, PD, PD, PD, PD, PD, PD]),
    "pgd_grid_posterior_many": (C.c_int, [H, PD, C.c_int, C.c_int, PD, PD, PD, I64, PD, PI32, C.c_int, PD, PD, C.c_int, PD, PI64, PD, PD, PD]),
    "pgd_postmany_data_block": (C.c_int, [C.c_int]),
    "pgd_design_update": (C.c_int, [H, PD, PD, C.c_int, C.c_int, PD, PD, PI32, C.c_int, PD, H, PD]),
    "pgd_design_gains": (C.c_int, [H, PD, I64, C.c_int, C.c_int, PD, PD, PI32, C.c_int, PD, H, PD]),
    "pgd_vec_ratio": (C.c_int, [H, H, H, H, C.c_double]),
    "pgd_pcg_solve": (C.c_int, [H, H, H, H, F64, F64, C.c_int, C.POINTER(C.c_int), PD]),
    "pgd_pcg_last_form": (C.c_int, [H, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pgd_band_solve": (C.c_int, [H, H, H, H]),
    "pgd_slots_ptr": (C.c_int, [H, C.POINTER(VP)]),
    "pgd_slots_download": (C.c_int, [H, PD, C.c_int, C.c_int]),
    "pgd_slots_upload": (C.c_int, [H, PD, C.c_int, C.c_int]),
    "pgd_flags_reset": (C.c_int, [H]),
    "pgd_flags_download": (C.c_int, [H, PI32, PI32, PI32]),
    "pgd_op_diag_inv": (C.c_int, [H, H, H]),
    "pgd_spmv_dot_slot": (C.c_int, [H, H, H, H, H, I64, I64, C.c_int]),
    "pgd_pcg_init_slot": (C.c_int, [H, H, H, H, H, H, H, I64, I64, C.c_int]),
    "pgd_pcg_tol_slot": (C.c_int, [H, F64, F64, C.c_int, C.c_int, C.c_int]),
    "pgd_pcg_xr_slot": (C.c_int, [H, H, H, H, H, H, H, I64, I64, C.c_int, C.c_int, C.c_int]),
    "pgd_pcg_check_slot": (C.c_int, [H, C.c_int, C.c_int]),
    "pgd_pcg_p_slot": (C.c_int, [H, H, H, I64, I64, C.c_int, C.c_int]),
    "pgd_cg_init_slot": (C.c_int, [H, H, H, H, H, H, H, H, I64, I64, C.c_int]),
    "pgd_cg_update_slot": (C.c_int, [H, H, H, H, H, H, H, H, I64, I64, C.c_int]),
    "pgd_cg_scalars_slot": (C.c_int, [H, C.c_int, C.c_int, F64, F64]),
    "pgd_comm_bind_callbacks": (C.c_int, [H, HALO_FN, ALLREDUCE_FN, VP, C.c_int, C.c_int]),
    "pgd_comm_unique_id": (C.c_int, [H, PU8]),
    "pgd_comm_bind_rccl": (C.c_int, [H, PU8, C.c_int, C.c_int]),
    "pgd_comm_overlap": (C.c_int, [H, C.c_int, C.POINTER(C.c_int)]),
    "pgd_comm_unbind": (C.c_int, [H]),
    "pgd_comm_timeout": (C.c_int, [H, F64]),
    "pgd_comm_prof": (C.c_int, [H, C.c_int, PD]),
    "pgd_comm_info": (C.c_int, [H, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pgd_comm_halo": (C.c_int, [H, H, I64, I64, I64, I64]),
    "pgd_comm_allreduce_slots": (C.c_int, [H, C.c_int, C.c_int]),
    "pgd_comm_push_export": (C.c_int, [H, I64, I64, I64, I64, I64, PU8]),
    "pgd_comm_push_attach": (C.c_int, [H, PU8, PU8, C.POINTER(C.c_int)]),
    "pgd_comm_push": (C.c_int, [H, C.c_int, C.POINTER(C.c_int)]),
    "pgd_comm_allreduce_attach": (C.c_int, [H, PU8, C.POINTER(C.c_int)]),
    "pgd_comm_allreduce_direct": (C.c_int, [H, C.c_int, C.POINTER(C.c_int)]),
    "pgd_pcg_solve_sharded": (C.c_int, [H, H, H, H, I64, I64, I64, I64, F64, F64, C.c_int, C.POINTER(C.c_int), PD]),
    "pgd_op_symmetrize": (C.c_int, [H, H, C.POINTER(C.c_int)]),
    "pgd_op_classify": (C.c_int, [H, H, C.POINTER(C.c_int)]),
    "pgd_tune": (C.c_int, [H, C.c_int, I64]),
    "pgd_prof_enable": (C.c_int, [H, C.c_int]),
    "pgd_prof_read": (C.c_int, [H, PI64, PD, PD]),
    "pgd_prof_read_own": (C.c_int, [H, PD]),
    "pgd_prof_read_update": (C.c_int, [H, PI64, PD, PD]),
    "pgd_prof_read_dropped": (C.c_int, [H, PI64]),
    "pgd_prof_event_overhead": (C.c_int, [H, PD]),
    "pgd_kernel_counts": (C.c_int, [H, PI64, C.c_int]),
    "pgd_pcg_recompute_counts": (C.c_int, [H, PI64]),
    "pgd_pcg_fused_counts": (C.c_int, [H, PI64]),
    "pgd_classify_counts": (C.c_int, [H, PI64, PI64]),
    "pgd_mg_counts": (C.c_int, [H, PI64, PI64]),
    "pgd_vmg_counts": (C.c_int, [H, PI64, PI64, PI64]),
    "pgd_vmg_times": (C.c_int, [H, C.POINTER(C.c_double), PI64]),
    "pgd_cmg_counts": (C.c_int, [H, PI64, PI64, PI64]),
    "pgd_cmg_times": (C.c_int, [H, C.POINTER(C.c_double), PI64]),
    "pgd_pmg_counts": (C.c_int, [H, PI64, PI64, PI64]),
    "pgd_pmg_times": (C.c_int, [H, C.POINTER(C.c_double), PI64]),
    "pgd_pmg_coarse": (C.c_int, [H, C.c_int, PD, PU8]),
    "pgd_bdia_counts": (C.c_int, [H, PI64, PI64, PI64]),
    "pgd_bdia_times": (C.c_int, [H, C.POINTER(C.c_double)]),
    "pgd_p2lat_counts": (C.c_int, [H, PI64, PI64, PI64]),
    "pgd_p2lat_times": (C.c_int, [H, C.POINTER(C.c_double)]),
    "pgd_calib_stream": (C.c_int, [H, H, C.c_int, C.c_int]),
    "pgd_points_locate": (C.c_int, [H, H, PD, I64, F64, PH]),
    "pgd_points_from": (C.c_int, [H, H, PI32, PD, I64, PH]),
    "pgd_points_download": (C.c_int, [H, H, PI32, PD]),
    "pgd_points_info": (C.c_int, [H, H, PI64, C.POINTER(C.c_int), PI64]),
    "pgd_points_last_path": (C.c_int, [H, C.POINTER(C.c_int)]),
    "pgd_points_index_info": (C.c_int, [H, H, PI64]),
    "pgd_points_index_download": (C.c_int, [H, H, PI32, PI32, PD]),
    "pgd_points_index_drop": (C.c_int, [H, H]),
    "pgd_points_sample": (C.c_int, [H, H, H, H, C.c_int, H]),
    "pgd_points_free": (C.c_int, [H, H]),
    "pgd_timer_start": (C.c_int, [H]),
    "pgd_timer_stop": (C.c_int, [H, PD]),
}

NSLOTS = 64
EVAL_STATS, EVAL_ENVELOPE, EVAL_EXCEED, EVAL_FIELDS = 1, 2, 4, 8      # PGD_EVAL_* (include/pgd_amd.h)
EVAL_Q_NORM, EVAL_Q_VALUE, EVAL_Q_EIG_MAX, EVAL_Q_EIG_MIN, EVAL_Q_EIG_SPREAD = range(5)      # pgd_eval_quantity
TUNE_EVAL_VARIANT, TUNE_EVAL_GRID_MAX, TUNE_EVAL_SAMPLE_CHUNK = 50, 51, 52
TUNE_BLOCK_STORAGE = 54
TUNE_PCG_FOLD_MARCH, TUNE_PCG_SCALAR_S, TUNE_PCG_FUSED_MARCH = 55, 56, 57
TUNE_SPMV_BLOCK_DIA = 58
TUNE_SPMV_P2_LATTICE = 59
TUNE_LOCATE_LATTICE, TUNE_LOCATE_GRID_MAX = 60, 61
TUNE_LOCATE_INDEX, TUNE_LOCATE_INDEX_TARGET = 66, 67
TUNE_GRAM_VARIANT, TUNE_GRAM_GRID_MAX = 62, 63
GRAM_KMAX = 128            # vectors per side and call of pgd_vec_gram
TUNE_QUAD_VARIANT, TUNE_QUAD_GRID_MAX = 64, 65
QUAD_KMAX, QUAD_NQMAX = 256, 64   # modes and forms per call of pgd_quad_forms
QUAD_CLAMP = 1
TUNE_MISFIT_VARIANT, TUNE_MISFIT_GRID_MAX, TUNE_POST_VARIANT, TUNE_POST_GRID_MAX = 68, 69, 70, 71
POST_KMAX, POST_MMAX, POST_DMAX, POST_COEF_KMAX = 256, 256, 6, 64   # modes, rows and dimensions of pgd_grid_misfit; modes of PGD_POST_COEF
POST_MARGINALS, POST_THETA, POST_COEF = 1, 2, 4                     # PGD_POST_* (include/pgd_amd.h)
TUNE_POSTMANY_VARIANT, TUNE_POSTMANY_GRID_MAX, TUNE_POSTMANY_SKIP = 72, 73, 74
POSTMANY_KMAX, POSTMANY_MMAX = 64, 64                               # modes and rows of pgd_grid_posterior_many
TUNE_DESIGN_VARIANT, TUNE_DESIGN_GRID_MAX = 75, 76
DESIGN_KMAX, DESIGN_RMAX = 64, 3                                    # modes and rows per candidate of pgd_design_gains
LOCATE_TILE = 32                                    # points per launch of the general location kernel (LOC_PT, csrc/pgd_locate.hip)
LOCATE_PATH_GENERAL, LOCATE_PATH_LATTICE = 1, 2     # pgd_points_last_path
LOCATE_PATH_INDEX = 3                               # ... the bin index (TUNE_LOCATE_INDEX)
LOCATE_INDEX_TOL = 2.0 ** -10                       # the bin index serves tolerances up to here (LOC_INDEX_TOL, csrc/pgd_locate.hip)
BLOCK_F32, BLOCK_F64, BLOCK_MAXK = 0, 1, 64                                           # PGD_BLOCK_* (include/pgd_amd.h)


ERR_TIMEOUT, ERR_PEER = -7, -8          # PGD_ERR_TIMEOUT, PGD_ERR_PEER (include/pgd_amd.h)


class PgdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libpgd_amd error {code}: {msg}")
        self.code = code


_lib = None


def load(path: Path | None = None):
    """dlopen libpgd_amd.so and type every entry point.  Raises if it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path else LIB_PATH
    if not p.exists():
        raise RuntimeError(
            f"{p} not found: build the HIP library first (python -m pgdrome_amd.build). "
            "pgdrome_amd has no CPU fallback.")
    _preload_hip_runtime()
    lib = C.CDLL(str(p))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError if the header and the library disagree
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64.so; if libpgd_amd.so pulls in
    the system copy first, a later `import torch` (needed for the RCCL path) finds the device taken and
    reports "No HIP GPUs are available".  Loading torch's copy first (without importing torch) makes both
    resolve to the same runtime whatever the import order."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = Path(list(spec.submodule_search_locations)[0]) / "lib" / "libamdhip64.so"
    if cand.exists():
        try:
            C.CDLL(str(cand), mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def dptr(a: np.ndarray):
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(PD)


def iptr(a: np.ndarray):
    assert a.dtype == np.int32 and a.flags.c_contiguous
    return a.ctypes.data_as(PI32)


class Context:
    """One device context; thin, checked wrappers around the C entry points."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self.lib = load()
        if self.lib.pgd_device_count() <= 0:
            raise RuntimeError("pgdrome_amd: no HIP device visible (no CPU fallback exists)")
        h = H(0)
        rc = self.lib.pgd_ctx_create(device, VP(stream) if stream else None, C.byref(h))
        if rc != 0:
            raise PgdError(rc, self.lib.pgd_last_error(0).decode())
        self.h = h.value
        self.device = device
        self._block_k = {}            # column blocks of this context: handle -> k
        self._locate_index = 0        # the value of TUNE_LOCATE_INDEX (tune keeps it: points_locate restores it)

    def close(self):
        if getattr(self, "h", 0):
            self.lib.pgd_ctx_destroy(self.h)
            self.h = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            raise PgdError(rc, self.lib.pgd_last_error(self.h).decode())

    def sync(self):
        self._ck(self.lib.pgd_sync(self.h))

    # ---- meshes
    def mesh_upload(self, coords, cells):
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        cells = np.ascontiguousarray(cells, dtype=np.int32)
        if coords.ndim == 1:
            coords = coords.reshape(-1, 1)
        m = H(0)
        self._ck(self.lib.pgd_mesh_upload(self.h, dptr(coords), coords.shape[0], coords.shape[1],
                                          iptr(cells), cells.shape[0], cells.shape[1], C.byref(m)))
        return m.value

    def mesh_blocked(self, mesh, ncomp):
        m = H(0)
        self._ck(self.lib.pgd_mesh_blocked(self.h, mesh, int(ncomp), C.byref(m)))
        return m.value

    def mesh_p2_bind(self, p2_mesh, p1_mesh, edge_vertices):
        """Bind a scalar P2 layout on tetrahedra to the box lattice of its vertices (pgd_mesh_p2_bind): True where the checks pass."""
        ev = np.ascontiguousarray(edge_vertices, dtype=np.int32).reshape(-1, 2)
        ok = C.c_int(0)
        self._ck(self.lib.pgd_mesh_p2_bind(self.h, p2_mesh, p1_mesh, iptr(ev), ev.shape[0], C.byref(ok)))
        return bool(ok.value)

    def atom_embed(self, bmesh, src, cv, cu, coef=1.0, dst=0):
        out = H(0)
        self._ck(self.lib.pgd_atom_embed(self.h, bmesh, src, int(cv), int(cu), float(coef), int(dst), C.byref(out)))
        return out.value

    def mesh_info(self, mesh):
        nv, nc, nnz = I64(), I64(), I64()
        mr, kl, ku = I32(), I32(), I32()
        self._ck(self.lib.pgd_mesh_info(self.h, mesh, C.byref(nv), C.byref(nc), C.byref(nnz),
                                        C.byref(mr), C.byref(kl), C.byref(ku)))
        return dict(nv=nv.value, nc=nc.value, nnz=nnz.value, max_row=mr.value, kl=kl.value, ku=ku.value)

    def mesh_pattern(self, mesh):
        info = self.mesh_info(mesh)
        rp = np.empty(info["nv"] + 1, dtype=np.int32)
        cols = np.empty(max(info["nnz"], 1), dtype=np.int32)
        self._ck(self.lib.pgd_mesh_pattern_download(self.h, mesh, iptr(rp), iptr(cols)))
        return rp, cols[: info["nnz"]]

    def mesh_sym_info(self, mesh):
        w, nx, ny = I32(), I32(), I32()
        self._ck(self.lib.pgd_mesh_sym_info(self.h, mesh, C.byref(w), C.byref(nx), C.byref(ny)))
        return {"slots": w.value, "nx": nx.value, "ny": ny.value}

    def mesh_lattice(self, mesh):
        """(is_lattice, steps[3]) of pgd_mesh_lattice."""
        flag, steps = I32(), np.zeros(3)
        self._ck(self.lib.pgd_mesh_lattice(self.h, mesh, C.byref(flag), dptr(steps)))
        return bool(flag.value), steps

    def mesh_dict_count(self, mesh):
        n = I32()
        self._ck(self.lib.pgd_mesh_dict_count(self.h, mesh, C.byref(n)))
        return n.value

    def mesh_free(self, mesh):
        self._ck(self.lib.pgd_mesh_free(self.h, mesh))

    # ---- vectors
    def vec_alloc(self, n):
        v = H(0)
        self._ck(self.lib.pgd_vec_alloc(self.h, int(n), C.byref(v)))
        return v.value

    def vec_from(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        v = self.vec_alloc(a.size)
        self.vec_upload(v, a)
        return v

    def vec_free(self, v):
        self._ck(self.lib.pgd_vec_free(self.h, v))

    def vec_size(self, v):
        n = I64()
        self._ck(self.lib.pgd_vec_size(self.h, v, C.byref(n)))
        return n.value

    def vec_upload(self, v, a, offset=0):
        a = np.ascontiguousarray(a, dtype=np.float64)
        self._ck(self.lib.pgd_vec_upload(self.h, v, dptr(a), int(offset), a.size))

    def vec_download(self, v, offset=0, count=None):
        if count is None:
            count = self.vec_size(v) - offset
        out = np.empty(count, dtype=np.float64)
        self._ck(self.lib.pgd_vec_download(self.h, v, dptr(out), int(offset), int(count)))
        return out

    def vec_ptr(self, v):
        p = VP()
        self._ck(self.lib.pgd_vec_ptr(self.h, v, C.byref(p)))
        return p.value

    def vec_fill(self, v, a):
        self._ck(self.lib.pgd_vec_fill(self.h, v, float(a)))

    def vec_copy(self, dst, src):
        self._ck(self.lib.pgd_vec_copy(self.h, dst, src))

    def vec_copy_range(self, dst, dst_off, src, src_off, count):
        """dst[dst_off : dst_off + count] = src[src_off : src_off + count] on the stream."""
        self._ck(self.lib.pgd_vec_copy_range(self.h, dst, int(dst_off), src, int(src_off), int(count)))

    def vec_scale(self, v, a):
        self._ck(self.lib.pgd_vec_scale(self.h, v, float(a)))

    def vec_mul(self, y, a, x):
        self._ck(self.lib.pgd_vec_mul(self.h, y, a, x))

    def vec_axpy(self, y, a, x):
        self._ck(self.lib.pgd_vec_axpy(self.h, y, float(a), x))

    def vec_lincomb(self, y, xs, coefs):
        k = len(xs)
        arr = (H * max(k, 1))(*[int(x) for x in xs])
        cf = np.ascontiguousarray(coefs, dtype=np.float64)
        self._ck(self.lib.pgd_vec_lincomb(self.h, y, arr, dptr(cf) if k else None, k))

    # ---- column blocks (pgd_block.hip)
    def block_storage(self):
        """BLOCK_F32 / BLOCK_F64 as PGD_TUNE_BLOCK_STORAGE selects for the spectral start space, None: separate vectors."""
        d = C.c_int()
        self._ck(self.lib.pgd_block_storage(self.h, C.byref(d)))
        return d.value if d.value >= 0 else None

    def block_create(self, n, k, dtype):
        b = H(0)
        self._ck(self.lib.pgd_block_create(self.h, int(n), int(k), int(dtype), C.byref(b)))
        self._block_k[b.value] = int(k)      # (the per-solve calls below need it: no pgd_block_info round trip)
        return b.value

    def block_free(self, b):
        self._ck(self.lib.pgd_block_free(self.h, b))
        self._block_k.pop(b, None)

    def block_info(self, b):
        n, k, d, nb = I64(), C.c_int(), C.c_int(), I64()
        self._ck(self.lib.pgd_block_info(self.h, b, C.byref(n), C.byref(k), C.byref(d), C.byref(nb)))
        return {"n": n.value, "k": k.value, "dtype": ("fp32", "f64")[d.value], "bytes": nb.value}

    def block_set_column(self, b, j, v):
        self._ck(self.lib.pgd_block_set_column(self.h, b, int(j), v))

    def block_get_column(self, b, j, v):
        self._ck(self.lib.pgd_block_get_column(self.h, b, int(j), v))

    def block_dots(self, b, r, lo=0, hi=-1):
        """[Y_j . r for every column j] over [lo, hi): one pass over the block, one host synchronisation."""
        out = np.zeros(BLOCK_MAXK, dtype=np.float64)
        self._ck(self.lib.pgd_block_dots(self.h, b, r, int(lo), int(hi), dptr(out)))
        return out[: self._block_k[b]].copy()

    def block_combine(self, b, coefs, base, x):
        """x = base + Y coefs (base: a vector, possibly x itself, or 0 / None for none)."""
        if len(coefs) != self._block_k[b]:
            raise ValueError("block_combine: one coefficient per column")
        cf = np.zeros(BLOCK_MAXK, dtype=np.float64)
        cf[: len(coefs)] = coefs
        self._ck(self.lib.pgd_block_combine(self.h, b, dptr(cf), int(base or 0), x))

    def vec_lincomb_inplace(self, y, xs, coefs):
        """vec_lincomb where xs[0] may be y itself (at most 64 terms)."""
        k = len(xs)
        arr = (H * max(k, 1))(*[int(x) for x in xs])
        cf = np.ascontiguousarray(coefs, dtype=np.float64)
        self._ck(self.lib.pgd_vec_lincomb_inplace(self.h, y, arr, dptr(cf) if k else None, k))

    def _eval_batch(self, name, fn, q, modes, coefs, stats, env_min, env_max, exceed, threshold, fields, lead=()):
        """The marshalling of ``eval_batch`` (``q`` = ()), ``eval_batch_norm`` (``q`` = (planes,)) and ``eval_batch_grad`` (``q`` = (L,
        planes, scale), ``lead`` = (mesh,)): ``fn`` takes ``lead`` after the context and ``q`` after k."""
        k = len(modes)
        cf = np.ascontiguousarray(coefs, dtype=np.float64)
        if cf.ndim != 2 or cf.shape[0] != k:
            raise ValueError("%s: coefs must have shape (len(modes), samples), got %r for %d modes" % (name, cf.shape, k))
        s = cf.shape[1]
        want = (EVAL_STATS if stats else 0) | (EVAL_ENVELOPE if (env_min or env_max) else 0) | \
               (EVAL_EXCEED if exceed else 0) | (EVAL_FIELDS if fields else 0)
        arr = (H * max(k, 1))(*[int(x) for x in modes])
        out = np.empty((3, s), dtype=np.float64) if stats else None
        self._ck(fn(self.h, *lead, arr, k, *q, dptr(cf) if cf.size else None, s, want, float(threshold),
                    dptr(out) if stats else None, int(env_min), int(env_max), int(exceed), int(fields)))
        return out

    def eval_batch(self, modes, coefs, stats=True, env_min=0, env_max=0, exceed=0, threshold=0.0, fields=0):
        """pgd_eval_batch: all samples (columns of ``coefs``, shape (k, s)) of u = sum_t coefs[t] modes[t] in one pass over
        the modes.  Outputs are requested by passing their vectors (``stats``: a flag); returns the (3, s) array of
        per-sample min / max / max |.| or None."""
        return self._eval_batch("eval_batch", self.lib.pgd_eval_batch, (), modes, coefs, stats, env_min, env_max, exceed, threshold, fields)

    def eval_batch_norm(self, modes, q, coefs, stats=True, env_min=0, env_max=0, exceed=0, threshold=0.0, fields=0):
        """pgd_eval_batch_norm: eval_batch on modes of ``q`` planes each, the value of an entry being the Euclidean norm over its
        planes of the combined planes.  Same arguments and return value as ``eval_batch``; the outputs have len(mode) / q entries."""
        return self._eval_batch("eval_batch_norm", self.lib.pgd_eval_batch_norm, (int(q),), modes, coefs, stats, env_min, env_max,
                                exceed, threshold, fields)

    def eval_batch_grad(self, mesh, modes, L, coefs, scale=0, stats=True, env_min=0, env_max=0, exceed=0, threshold=0.0, fields=0):
        """pgd_eval_batch_grad: ``cell_gradient`` of every nodal mode and ``eval_batch_norm`` on the planes in one call that stores no
        planes.  ``mesh``, ``L`` (q, ncomp * gdim), ``scale`` as ``cell_gradient``; the rest and the return value as ``eval_batch``,
        the outputs with one entry per cell."""
        L = np.ascontiguousarray(L, dtype=np.float64)
        if L.ndim != 2:
            raise ValueError("eval_batch_grad: L is a (q, ncomp * gdim) matrix")
        return self._eval_batch("eval_batch_grad", self.lib.pgd_eval_batch_grad, (dptr(L) if L.size else None, L.shape[0], int(scale or 0)),
                                modes, coefs, stats, env_min, env_max, exceed, threshold, fields, lead=(int(mesh),))

    def eval_batch_quantity(self, modes, q, kind, coefs, stats=True, env_min=0, env_max=0, exceed=0, threshold=0.0, fields=0):
        """pgd_eval_batch_quantity: ``eval_batch_norm`` with the value of ``kind`` (EVAL_Q_*: the norm, the signed value of one plane,
        the largest / smallest eigenvalue of the symmetric tensor of q = 6 or 4 planes, or their difference) in the place of the norm."""
        return self._eval_batch("eval_batch_quantity", self.lib.pgd_eval_batch_quantity, (int(q), int(kind)), modes, coefs, stats, env_min,
                                env_max, exceed, threshold, fields)

    def eval_batch_grad_quantity(self, mesh, modes, L, kind, coefs, scale=0, stats=True, env_min=0, env_max=0, exceed=0, threshold=0.0,
                                 fields=0):
        """pgd_eval_batch_grad_quantity: ``eval_batch_grad`` with the value of ``kind`` as ``eval_batch_quantity`` has it."""
        L = np.ascontiguousarray(L, dtype=np.float64)
        if L.ndim != 2:
            raise ValueError("eval_batch_grad_quantity: L is a (q, ncomp * gdim) matrix")
        return self._eval_batch("eval_batch_grad_quantity", self.lib.pgd_eval_batch_grad_quantity,
                                (dptr(L) if L.size else None, L.shape[0], int(kind), int(scale or 0)), modes, coefs, stats, env_min, env_max,
                                exceed, threshold, fields, lead=(int(mesh),))

    def eval_batch_grad_p2_quantity(self, mesh, modes, lam, L, kind, coefs, scale=0, stats=True, env_min=0, env_max=0, exceed=0,
                                    threshold=0.0, fields=0):
        """pgd_eval_batch_grad_p2_quantity: ``eval_batch_grad_p2`` with the value of ``kind`` as ``eval_batch_quantity`` has it."""
        lam, L = self._p2_points("eval_batch_grad_p2_quantity", lam, L)
        return self._eval_batch("eval_batch_grad_p2_quantity", self.lib.pgd_eval_batch_grad_p2_quantity,
                                (dptr(lam) if lam.size else None, lam.shape[0], dptr(L) if L.size else None, L.shape[0], int(kind),
                                 int(scale or 0)), modes, coefs, stats, env_min, env_max, exceed, threshold, fields, lead=(int(mesh),))

    def eval_norm_last_shape(self):
        """(entries per workgroup, staged) of the last eval_batch_norm / eval_batch_grad that launched; staged: 1 = the planes of a row block in at most
        64 KiB of LDS, 2 = in more, 0 = read from global memory (pgd_eval_norm_last_shape)."""
        rows, staged = C.c_int(), C.c_int()
        self._ck(self.lib.pgd_eval_norm_last_shape(self.h, C.byref(rows), C.byref(staged)))
        return rows.value, staged.value

    def cell_gradient(self, mesh, u, L, out, scale=0):
        """pgd_cell_gradient: out[i * nc + cell] = scale[cell] * sum_j L[i, j] g[j] for the P1 field ``u`` of the layout ``mesh``
        (scalar or blocked), g[c * gdim + a] = d u_c / d x_a; ``L``: (q, ncomp * gdim); ``scale``: a vector of one entry per cell, or 0."""
        L = np.ascontiguousarray(L, dtype=np.float64)
        if L.ndim != 2:
            raise ValueError("cell_gradient: L is a (q, ncomp * gdim) matrix")
        self._ck(self.lib.pgd_cell_gradient(self.h, mesh, u, dptr(L) if L.size else None, L.shape[0], int(scale or 0), out))

    @staticmethod
    def _p2_points(name, lam, L):
        lam, L = np.ascontiguousarray(lam, dtype=np.float64), np.ascontiguousarray(L, dtype=np.float64)
        if lam.ndim != 2 or L.ndim != 2:
            raise ValueError("%s: lam is a (npt, gdim + 1) matrix, L a (q, ncomp * gdim) matrix" % name)
        return lam, L

    def cell_gradient_p2(self, mesh, u, lam, L, out, scale=0):
        """pgd_cell_gradient_p2: ``cell_gradient`` for the P2 field ``u`` of the P2 layout ``mesh`` at the points ``lam`` (npt, gdim + 1:
        barycentric coordinates) of every cell: out[(i * npt + a) * nc + cell] is plane i at point a."""
        lam, L = self._p2_points("cell_gradient_p2", lam, L)
        self._ck(self.lib.pgd_cell_gradient_p2(self.h, mesh, u, dptr(lam) if lam.size else None, lam.shape[0], dptr(L) if L.size else None,
                                               L.shape[0], int(scale or 0), out))

    def eval_batch_grad_p2(self, mesh, modes, lam, L, coefs, scale=0, stats=True, env_min=0, env_max=0, exceed=0, threshold=0.0, fields=0):
        """pgd_eval_batch_grad_p2: ``eval_batch_grad`` on nodal P2 modes at the points ``lam`` of every cell; the outputs have npt *
        cells entries, point-major."""
        lam, L = self._p2_points("eval_batch_grad_p2", lam, L)
        return self._eval_batch("eval_batch_grad_p2", self.lib.pgd_eval_batch_grad_p2,
                                (dptr(lam) if lam.size else None, lam.shape[0], dptr(L) if L.size else None, L.shape[0], int(scale or 0)),
                                modes, coefs, stats, env_min, env_max, exceed, threshold, fields, lead=(int(mesh),))

    # ---- point sets
    def points_locate(self, mesh, pts, tol=1e-10, index=False):
        """pgd_points_locate: the point set handle of ``pts`` (P, gdim) on the layout ``mesh``; a point outside gets cell -1.
        ``index``: True / False set TUNE_LOCATE_INDEX to 1 / 0 around the call and restore it (the bin index of the mesh is used, and
        built where there is none, wherever it applies: 2-D and 3-D, tol <= LOCATE_INDEX_TOL, no lattice path); None leaves the knob
        as ``tune`` set it."""
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        if pts.ndim != 2:
            raise ValueError("points_locate: pts is a (points, gdim) array")
        out = H(0)
        before = self._locate_index
        if index is not None:
            self.tune(TUNE_LOCATE_INDEX, 1 if index else 0)
        try:
            self._ck(self.lib.pgd_points_locate(self.h, mesh, dptr(pts) if pts.size else None, pts.shape[0], float(tol), C.byref(out)))
        finally:
            if index is not None:
                self.tune(TUNE_LOCATE_INDEX, before)
        return out.value

    def points_from(self, mesh, cells, lam):
        """pgd_points_from: the point set of known cells (P,) and barycentric coordinates (P, gdim + 1); a cell may be -1."""
        cells = np.ascontiguousarray(cells, dtype=np.int32)
        lam = np.ascontiguousarray(lam, dtype=np.float64)
        if cells.ndim != 1 or lam.ndim != 2 or lam.shape[0] != cells.shape[0]:
            raise ValueError("points_from: cells (P,) and lam (P, gdim + 1)")
        out = H(0)
        self._ck(self.lib.pgd_points_from(self.h, mesh, iptr(cells) if cells.size else None, dptr(lam) if lam.size else None,
                                          cells.shape[0], C.byref(out)))
        return out.value

    def points_info(self, points):
        """(number of points, gdim, first point outside the mesh or -1) of a point set."""
        n, g, first = I64(0), C.c_int(0), I64(0)
        self._ck(self.lib.pgd_points_info(self.h, points, C.byref(n), C.byref(g), C.byref(first)))
        return n.value, g.value, first.value

    def points_download(self, points):
        """(cells (P,) int32, lam (P, gdim + 1)) of a point set."""
        n, g, _ = self.points_info(points)
        cells, lam = np.empty(n, dtype=np.int32), np.empty((n, g + 1), dtype=np.float64)
        self._ck(self.lib.pgd_points_download(self.h, points, iptr(cells), dptr(lam)))
        return cells, lam

    def points_last_path(self):
        """What the last points_locate ran: 0 nothing, LOCATE_PATH_GENERAL, LOCATE_PATH_LATTICE, LOCATE_PATH_INDEX."""
        path = C.c_int(0)
        self._ck(self.lib.pgd_points_last_path(self.h, C.byref(path)))
        return path.value

    def points_index_info(self, mesh):
        """pgd_points_index_info: the bin index of the mesh as a dict - built, builds, n (bins per axis), entries, longest, bytes; all
        zero before a build and after a drop."""
        out = (I64 * 8)()
        self._ck(self.lib.pgd_points_index_info(self.h, mesh, out))
        v = [int(x) for x in out]
        return dict(built=v[0], builds=v[1], n=(v[2], v[3], v[4]), entries=v[5], longest=v[6], bytes=v[7])

    def points_index_download(self, mesh):
        """pgd_points_index_download: (bin_ptr (bins + 1,), bin_cells (entries,), origin (3,), inv (3,), n (3,) int64)."""
        info = self.points_index_info(mesh)
        bins = info["n"][0] * info["n"][1] * info["n"][2]
        bin_ptr, bin_cells = np.zeros(bins + 1, dtype=np.int32), np.zeros(max(info["entries"], 1), dtype=np.int32)
        geom = np.zeros(9)
        self._ck(self.lib.pgd_points_index_download(self.h, mesh, iptr(bin_ptr), iptr(bin_cells), dptr(geom)))
        return bin_ptr, bin_cells[:info["entries"]], geom[:3].copy(), geom[3:6].copy(), geom[6:].astype(np.int64)

    def points_index_drop(self, mesh):
        """pgd_points_index_drop: frees the bin index of the mesh (nothing happens without one)."""
        self._ck(self.lib.pgd_points_index_drop(self.h, mesh))

    def points_sample(self, points, layout, u, out, gradient=False):
        """pgd_points_sample: the values (``gradient``: the gradients) of the nodal field ``u`` of ``layout`` at the points, into ``out``."""
        self._ck(self.lib.pgd_points_sample(self.h, points, layout, u, 1 if gradient else 0, out))

    def points_free(self, points):
        self._ck(self.lib.pgd_points_free(self.h, points))

    def vec_set(self, v, idx, val):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        val = np.ascontiguousarray(np.broadcast_to(np.asarray(val, dtype=np.float64), idx.shape))
        self._ck(self.lib.pgd_vec_set(self.h, v, iptr(idx), dptr(val), idx.size))

    def vec_dot(self, x, y, lo=0, hi=-1):
        out = F64()
        self._ck(self.lib.pgd_vec_dot(self.h, x, y, int(lo), int(hi), C.byref(out)))
        return out.value

    def vec_multidot(self, x, ys, lo=0, hi=-1):
        """[x . y for y in ys] over [lo, hi): one host synchronisation for up to 256 vectors."""
        k = len(ys)
        arr = (H * k)(*[int(v) for v in ys])
        out = np.zeros(k, dtype=np.float64)
        self._ck(self.lib.pgd_vec_multidot(self.h, x, arr, k, int(lo), int(hi), dptr(out)))
        return out

    def vec_multidot_pair(self, x0, x1, ys, lo=0, hi=-1):
        """([x0 . y for y in ys], [x1 . y for y in ys]) over [lo, hi): every y read once for both, one host synchronisation."""
        k = len(ys)
        arr = (H * k)(*[int(v) for v in ys])
        out = np.zeros(2 * k, dtype=np.float64)
        self._ck(self.lib.pgd_vec_multidot_pair(self.h, x0, x1, arr, k, int(lo), int(hi), dptr(out)))
        return out[:k], out[k:]

    def vec_gram(self, xs, ys=None, lo=0, hi=-1):
        """pgd_vec_gram: the (kx, ky) array of x_i . y_j over [lo, hi), every vector read once per call.  ``ys`` None: the
        symmetric block of ``xs`` with itself, symmetric bit for bit.  Families above 128 vectors go in blocks of at most 128 per
        side; a symmetric request computes the blocks on and above the diagonal and mirrors the others."""
        xs = [int(v) for v in xs]
        sym = ys is None
        ys = xs if sym else [int(v) for v in ys]
        kx, ky = len(xs), len(ys)
        out = np.zeros((kx, ky), dtype=np.float64)
        for i0 in range(0, kx, GRAM_KMAX):
            xb = xs[i0:i0 + GRAM_KMAX]
            xa = (H * len(xb))(*xb)
            for j0 in range(0, ky, GRAM_KMAX):
                if sym and j0 < i0:
                    continue
                yb = ys[j0:j0 + GRAM_KMAX]
                blk = np.zeros((len(xb), len(yb)), dtype=np.float64)
                if sym and j0 == i0:
                    self._ck(self.lib.pgd_vec_gram(self.h, xa, len(xb), None, len(xb), int(lo), int(hi), dptr(blk)))
                else:
                    ya = (H * len(yb))(*yb)
                    self._ck(self.lib.pgd_vec_gram(self.h, xa, len(xb), ya, len(yb), int(lo), int(hi), dptr(blk)))
                out[i0:i0 + len(xb), j0:j0 + len(yb)] = blk
                if sym and j0 > i0:
                    out[j0:j0 + len(yb), i0:i0 + len(xb)] = blk.T
        return out

    def quad_forms(self, modes, Q, outs=None, clamp=False):
        """pgd_quad_forms: f_i^T Q_q f_i at every entry i for the nq matrices ``Q`` (nq, k, k) or (k, k), every mode read once per
        call of at most 64 forms.  ``outs``: one vector handle or None per form (None: no field is stored).  Returns the arrays
        (min, max) over the entries of every form, of the values as stored (``clamp``: below 0 as 0)."""
        modes = [int(v) for v in modes]
        k = len(modes)
        Q = np.asarray(Q, dtype=np.float64)
        if Q.ndim == 2:
            Q = Q[None]
        if Q.ndim != 3 or Q.shape[1:] != (k, k) or Q.shape[0] < 1:
            raise ValueError(f"quad_forms: Q has shape {Q.shape}, (nq, {k}, {k}) is needed")
        nq = Q.shape[0]
        outs = [None] * nq if outs is None else list(outs)
        if len(outs) != nq:
            raise ValueError(f"quad_forms: {len(outs)} outputs for {nq} forms")
        ma = (H * k)(*modes)
        mn, mx = np.empty(nq), np.empty(nq)
        for q0 in range(0, nq, QUAD_NQMAX):
            qb = np.ascontiguousarray(Q[q0:q0 + QUAD_NQMAX])
            ob = [0 if o is None else int(o) for o in outs[q0:q0 + QUAD_NQMAX]]
            oa = (H * len(ob))(*ob)
            ext = np.zeros(2 * len(ob), dtype=np.float64)
            self._ck(self.lib.pgd_quad_forms(self.h, ma, k, dptr(qb), len(ob), QUAD_CLAMP if clamp else 0, oa, dptr(ext)))
            mn[q0:q0 + len(ob)] = ext[0::2]
            mx[q0:q0 + len(ob)] = ext[1::2]
        return mn, mx

    @staticmethod
    def _grid_tables(tables, k):
        """(concatenated tables, n): the k x n[d] tables of a grid one after the other, as the two grid calls take them."""
        tables = [np.ascontiguousarray(t, dtype=np.float64) for t in tables]
        for d, t in enumerate(tables):
            if t.ndim != 2 or t.shape[0] != k:
                raise ValueError(f"grid tables: table {d} has shape {t.shape}, ({k}, n) is needed")
        n = np.array([t.shape[1] for t in tables], dtype=np.int32)
        flat = tables[0].reshape(-1) if len(tables) == 1 else np.concatenate([t.reshape(-1) for t in tables])    # (one table: no copy)
        return np.ascontiguousarray(flat), n

    def grid_misfit(self, a, y, tables, chi2):
        """pgd_grid_misfit: chi2[s] = |y - a c(s)|^2 on the tensor grid of the ``tables`` (one (k, n[d]) array per dimension, last
        dimension fastest) into the vector ``chi2`` of prod n[d] entries.  Returns (min, lowest index of the min)."""
        a = np.ascontiguousarray(a, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        if a.ndim != 2 or a.shape[0] != y.size:
            raise ValueError(f"grid_misfit: a has shape {a.shape} for {y.size} data")
        m, k = a.shape
        flat, n = self._grid_tables(tables, k)
        mn, arg = F64(0.0), I64(0)
        self._ck(self.lib.pgd_grid_misfit(self.h, dptr(a), dptr(y), m, k, dptr(flat), iptr(n), len(n), chi2, C.byref(mn), C.byref(arg)))
        return mn.value, arg.value

    def grid_posterior(self, chi2, shift, n, weights, tables=None, abscissae=None, want=0):
        """pgd_grid_posterior: the sums of e_s = w_s exp(-(chi2[s] - shift) / 2) over the grid of ``n`` points per dimension;
        ``weights`` / ``abscissae``: one array per dimension, ``tables`` as in ``grid_misfit`` (only for POST_COEF).  Returns a dict:
        "Z", "sum_e2", and per bit of ``want`` "marginals" (a list of arrays), "theta1", "theta2", "coef1", "coef2"."""
        n = np.ascontiguousarray(n, dtype=np.int32).reshape(-1)
        nd = len(n)
        cat = lambda xs: np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in xs]))
        w = cat(weights)
        if len(weights) != nd or w.size != int(n.sum()):
            raise ValueError("grid_posterior: the weights do not match n")
        none = C.cast(None, PD)
        x = none
        if want & POST_THETA:
            xa = cat(abscissae)
            if len(abscissae) != nd or xa.size != w.size:
                raise ValueError("grid_posterior: the abscissae do not match n")
            x = dptr(xa)
        k, t = 0, none
        if want & POST_COEF:
            k = int(np.asarray(tables[0]).shape[0])
            flat, nt = self._grid_tables(tables, k)
            if not np.array_equal(nt, n):
                raise ValueError("grid_posterior: the tables do not match n")
            t = dptr(flat)
        sums = np.zeros(2)
        marg = np.zeros(w.size if want & POST_MARGINALS else 0)
        th1, th2 = np.zeros(nd), np.zeros((nd, nd))
        c1, c2 = np.zeros(k), np.zeros((k, k))
        opt = lambda arr, bit: dptr(arr) if want & bit else none
        self._ck(self.lib.pgd_grid_posterior(self.h, chi2, float(shift), t, iptr(n), nd, k, dptr(w), x, int(want), dptr(sums),
                                             opt(marg, POST_MARGINALS), opt(th1, POST_THETA), opt(th2, POST_THETA),
                                             opt(c1, POST_COEF), opt(c2, POST_COEF)))
        out = {"Z": float(sums[0]), "sum_e2": float(sums[1])}
        if want & POST_MARGINALS:
            out["marginals"] = np.split(marg, np.cumsum(n)[:-1])
        if want & POST_THETA:
            out["theta1"], out["theta2"] = th1, th2
        if want & POST_COEF:
            out["coef1"], out["coef2"] = c1, c2
        return out

    def postmany_data_block(self, ndim):
        """The data sets a wave of the matrix-unit kernel of ``grid_posterior_many`` holds for ``ndim`` dimensions."""
        return int(self.lib.pgd_postmany_data_block(int(ndim)))

    def grid_posterior_many(self, a, u, alpha, beta, tables, weights, abscissae=None, want=0):
        """pgd_grid_posterior_many: for every row j of ``u`` (nd, m) with the scalars ``alpha[j]``, ``beta[j]`` the misfits
        chi2[j, s] = beta_j - 2 u_j . (a c(s)) + alpha_j |a c(s)|^2 over the grid of the ``tables`` (as in ``grid_misfit``), reduced
        where they are formed.  Returns a dict of arrays of leading size nd: "chi2_min", "argmin", "Z", "sum_e2" and, with
        POST_THETA, "theta1" (nd, D), "theta2" (nd, D, D)."""
        a = np.ascontiguousarray(a, dtype=np.float64)
        u = np.ascontiguousarray(u, dtype=np.float64)
        if a.ndim != 2 or u.ndim != 2 or u.shape[1] != a.shape[0] or u.shape[0] < 1:
            raise ValueError(f"grid_posterior_many: a has shape {a.shape}, u has shape {u.shape}: (m, k) and (nd, m) are needed")
        m, k = a.shape
        nd = u.shape[0]
        alpha = np.ascontiguousarray(alpha, dtype=np.float64).reshape(-1)
        beta = np.ascontiguousarray(beta, dtype=np.float64).reshape(-1)
        if alpha.size != nd or beta.size != nd:
            raise ValueError(f"grid_posterior_many: {alpha.size} alpha and {beta.size} beta for {nd} data sets")
        flat, n = self._grid_tables(tables, k)
        D = len(n)
        cat = lambda xs: np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in xs]))
        w = cat(weights)
        if len(weights) != D or w.size != int(n.sum()):
            raise ValueError("grid_posterior_many: the weights do not match the tables")
        x = C.cast(None, PD)
        if want & POST_THETA:
            xa = cat(abscissae)
            if len(abscissae) != D or xa.size != w.size:
                raise ValueError("grid_posterior_many: the abscissae do not match the tables")
            x = dptr(xa)
        cmin, arg, sums = np.zeros(nd), np.zeros(nd, dtype=np.int64), np.zeros((nd, 2))
        th1, th2 = np.zeros((nd, D)), np.zeros((nd, D, D))
        self._ck(self.lib.pgd_grid_posterior_many(self.h, dptr(a), m, k, dptr(u), dptr(alpha), dptr(beta), nd, dptr(flat), iptr(n), D,
                                                  dptr(w), x, int(want), dptr(cmin), arg.ctypes.data_as(PI64), dptr(sums), dptr(th1),
                                                  dptr(th2)))
        out = {"chi2_min": cmin, "argmin": arg, "Z": sums[:, 0].copy(), "sum_e2": sums[:, 1].copy()}
        if want & POST_THETA:
            out["theta1"], out["theta2"] = th1, th2
        return out

    def _design_grid(self, who, tables, dtables, weights, k):
        flat, n = self._grid_tables(tables, k)
        dflat, dn = self._grid_tables(dtables, k)
        if not np.array_equal(n, dn):
            raise ValueError(f"{who}: the dtables do not match the tables")
        w = np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for x in weights]))
        if len(weights) != len(n) or w.size != int(n.sum()):
            raise ValueError(f"{who}: the weights do not match the tables")
        return flat, dflat, n, w

    def design_state(self, n):
        """A vector for the state of ``design_update`` / ``design_gains`` on the grid of ``n`` points per dimension: 2 nh S doubles."""
        D = len(n)
        return self.vec_alloc(D * (D + 1) * int(np.prod(n, dtype=np.int64)))

    def design_update(self, state, tables, dtables, weights, rows=None, h0=None):
        """pgd_design_update: H_s (= ``h0`` first, if given) += g g^T for the ``rows`` (R, k), W_s recomputed.  Returns
        (sum_s w_s log det H_s, the expected posterior covariance sum_s w_s H_s^-1 as a (D, D) matrix)."""
        k = int(np.asarray(tables[0]).shape[0])
        rows = np.zeros((0, k)) if rows is None else np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, k)
        flat, dflat, n, w = self._design_grid("design_update", tables, dtables, weights, k)
        D = len(n)
        none = C.cast(None, PD)
        hp = none
        if h0 is not None:
            h0 = np.ascontiguousarray(h0, dtype=np.float64)
            if h0.shape != (D, D):
                raise ValueError(f"design_update: h0 has shape {h0.shape}, ({D}, {D}) is needed")
            hp = dptr(h0)
        sums = np.zeros(1 + D * (D + 1) // 2)
        self._ck(self.lib.pgd_design_update(self.h, hp, dptr(rows) if rows.shape[0] else none, rows.shape[0], k, dptr(flat), dptr(dflat),
                                            iptr(n), D, dptr(w), state, dptr(sums)))
        cov = np.zeros((D, D))
        cov[np.triu_indices(D)] = sums[1:]
        return float(sums[0]), cov + np.triu(cov, 1).T

    def design_gains(self, a, R, state, tables, dtables, weights):
        """pgd_design_gains: the gains (in nats) of the M candidates whose R rows each are the rows of ``a`` (M R, k), at the state."""
        a = np.ascontiguousarray(a, dtype=np.float64)
        R = int(R)
        if a.ndim != 2 or R < 1 or a.shape[0] % R or a.shape[0] < R:
            raise ValueError(f"design_gains: a has shape {a.shape}, (M R, k) with R = {R} is needed")
        k = a.shape[1]
        flat, dflat, n, w = self._design_grid("design_gains", tables, dtables, weights, k)
        gains = np.zeros(a.shape[0] // R)
        self._ck(self.lib.pgd_design_gains(self.h, dptr(a), gains.size, R, k, dptr(flat), dptr(dflat), iptr(n), len(n), dptr(w), state,
                                           dptr(gains)))
        return gains

    def vec_ratio(self, out, num, den, floor=0.0):
        """pgd_vec_ratio: out = num / den where den > floor, 0 elsewhere (``out`` may be ``num``)."""
        self._ck(self.lib.pgd_vec_ratio(self.h, out, num, den, float(floor)))

    # ---- atoms / operators
    def atom_product_form(self, atom):
        """0: CSR kernels, 1: z-march over the diagonal form, 2: z-march over the atom's row classes."""
        f = C.c_int(0)
        self._ck(self.lib.pgd_atom_product_form(self.h, atom, C.byref(f)))
        return f.value

    def atom_assemble(self, mesh, kind, da=0, db=0, w=0):
        a = H(0)
        self._ck(self.lib.pgd_atom_assemble(self.h, mesh, int(kind), int(da), int(db), int(w), C.byref(a)))
        return a.value

    def atom_assemble_cells(self, mesh, kind, da, db, w, mask):
        """The atom of atom_assemble over the cells whose byte of `mask` (one per cell, upload order) is non-zero."""
        mask = np.ascontiguousarray(mask)
        if mask.ndim != 1 or mask.dtype.itemsize != 1:
            raise ValueError("mask: one byte per cell")
        mask = mask.view(np.uint8)
        a = H(0)
        self._ck(self.lib.pgd_atom_assemble_cells(self.h, mesh, int(kind), int(da), int(db), int(w),
                                                  mask.ctypes.data_as(PU8) if mask.size else None, mask.size, C.byref(a)))
        return a.value

    def atom_assemble_cellwise(self, mesh, kind, da, db, w, c, mask=None, nc=None):
        """The atom of atom_assemble with every cell's local matrix scaled by its entry of the device vector `c` (one per cell,
        upload order); mask: None = every cell, else one byte per cell as in atom_assemble_cells.  nc: the cell count
        (default: the mask's length, or the vector's)."""
        ptr = None
        if mask is not None:
            mask = np.ascontiguousarray(mask)
            if mask.ndim != 1 or mask.dtype.itemsize != 1:
                raise ValueError("mask: one byte per cell")
            mask = mask.view(np.uint8)
            ptr = mask.ctypes.data_as(PU8) if mask.size else None
            if nc is None:
                nc = mask.size
        if nc is None:
            nc = self.vec_size(c)
        a = H(0)
        self._ck(self.lib.pgd_atom_assemble_cellwise(self.h, mesh, int(kind), int(da), int(db), int(w), int(c), ptr, int(nc),
                                                     C.byref(a)))
        return a.value

    def atom_assemble_facets(self, mesh, facets):
        """int_Gamma phi_i phi_j ds over the facets: an (nf, nodes per facet) array of node ids of the layout."""
        facets = np.ascontiguousarray(facets, dtype=np.int32)
        if facets.ndim != 2:
            raise ValueError("facets: an (nf, nodes per facet) array")
        a = H(0)
        self._ck(self.lib.pgd_atom_assemble_facets(self.h, mesh, iptr(facets) if facets.size else None, facets.shape[0],
                                                   facets.shape[1], C.byref(a)))
        return a.value

    def atom_upload(self, mesh, vals):
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        a = H(0)
        self._ck(self.lib.pgd_atom_upload(self.h, mesh, dptr(vals), C.byref(a)))
        return a.value

    def atom_download(self, atom, nnz):
        out = np.empty(max(nnz, 1), dtype=np.float64)
        self._ck(self.lib.pgd_atom_download(self.h, atom, dptr(out)))
        return out[:nnz]

    def atom_free(self, a):
        self._ck(self.lib.pgd_atom_free(self.h, a))

    def op_combine(self, mesh, atoms, coefs, bc_dofs=None, op=0):
        n = len(atoms)
        arr = (H * n)(*[int(a) for a in atoms])
        cf = np.ascontiguousarray(coefs, dtype=np.float64)
        bc = np.ascontiguousarray(bc_dofs if bc_dofs is not None else [], dtype=np.int32)
        o = H(int(op))
        self._ck(self.lib.pgd_op_combine(self.h, mesh, arr, dptr(cf), n,
                                         iptr(bc) if bc.size else None, bc.size, C.byref(o)))
        return o.value

    def spmv(self, A, x, y, r0=0, r1=-1):
        self._ck(self.lib.pgd_spmv(self.h, A, x, y, int(r0), int(r1)))

    def bilinear(self, A, x, y, r0=0, r1=-1):
        out = F64()
        self._ck(self.lib.pgd_bilinear(self.h, A, x, y, int(r0), int(r1), C.byref(out)))
        return out.value

    def bilinear_many(self, A, x, ys, r0=0, r1=-1):
        n = len(ys)
        out = np.zeros(max(n, 1), dtype=np.float64)
        arr = (H * max(n, 1))(*[int(v) for v in ys])
        self._ck(self.lib.pgd_bilinear_many(self.h, A, x, arr, n, int(r0), int(r1), dptr(out)))
        return out[:n]

    def start_gram(self, A, vecs, b, r0=0, r1=-1):
        """(G, g): G[i, j] = v_i . (A v_j), g[j] = v_j . b over rows [r0, r1); one host synchronisation."""
        k = len(vecs)
        arr = (H * k)(*[int(v) for v in vecs])
        out = np.zeros(k * k + k, dtype=np.float64)
        self._ck(self.lib.pgd_start_gram(self.h, A, arr, k, b, int(r0), int(r1), dptr(out)))
        return out[:k * k].reshape(k, k).copy(), out[k * k:].copy()

    def start_residual(self, A, coefs, b, r):
        """r = b - sum_j coefs[j] (A v_j) from the products the start_gram call right before has left in the library."""
        cf = np.ascontiguousarray(coefs, dtype=np.float64)
        self._ck(self.lib.pgd_start_residual(self.h, A, int(cf.size), dptr(cf), b, r))

    def pcg_solve(self, op, b, x, rtol=1e-10, atol=0.0, maxit=10000):
        it = C.c_int()
        rel = F64()
        self._ck(self.lib.pgd_pcg_solve(self.h, op, b, x, float(rtol), float(atol), int(maxit),
                                        C.byref(it), C.byref(rel)))
        return it.value, rel.value

    PCG_FORMS = ("PRECOND", "TEXTBOOK", "TWO_LAUNCH", "FOLDED", "SINGLE_SYNC", "SINGLE_SYNC_RECOMPUTE", "DEFERRED_X", "PLAIN")
    PCG_PRECONDS = ("JACOBI", "MG", "VMG", "CMG", "PMG")

    def pcg_last_form(self):
        """(form, preconditioner) of the last pcg_solve by name (pgd_pcg_form / pgd_pcg_precond), (None, None) before the first."""
        f, p = C.c_int(), C.c_int()
        self._ck(self.lib.pgd_pcg_last_form(self.h, C.byref(f), C.byref(p)))
        return (self.PCG_FORMS[f.value] if f.value >= 0 else None, self.PCG_PRECONDS[p.value] if p.value >= 0 else None)

    # ---- the V-cycle on a z-slab of a row-sharded lattice (levels >= 1 whole on every rank)
    def mg_slab_setup(self, op, nz_global, z_first, own0, own1):
        """Entries of a level-1 vector where the slab V-cycle applies to this operator, else 0."""
        n1, ok = I64(0), C.c_int(0)
        self._ck(self.lib.pgd_mg_slab_setup(self.h, op, int(nz_global), int(z_first), int(own0), int(own1), C.byref(n1), C.byref(ok)))
        return int(n1.value) if ok.value else 0

    def mg_slab_fix_start(self, op, b, x, own0, own1):
        self._ck(self.lib.pgd_mg_slab_fix_start(self.h, op, b, x, int(own0), int(own1)))

    def mg_slab_down(self, r, t):
        self._ck(self.lib.pgd_mg_slab_down(self.h, r, t))

    def mg_slab_restrict(self, t, b1):
        self._ck(self.lib.pgd_mg_slab_restrict(self.h, t, b1))

    def mg_coarse(self, b1, x1):
        self._ck(self.lib.pgd_mg_coarse(self.h, b1, x1))

    def mg_slab_up(self, r, x1, t, z, slot=-1):
        """z = M r on the owned planes; r . z to the host (slot < 0) or into that scalar slot without a host synchronisation."""
        if slot >= 0:
            self._ck(self.lib.pgd_mg_slab_up(self.h, r, x1, t, z, int(slot), None))
            return None
        out = F64()
        self._ck(self.lib.pgd_mg_slab_up(self.h, r, x1, t, z, -1, C.byref(out)))
        return out.value

    def bicgstab(self, op, b, x, rtol=1e-10, atol=0.0, maxit=10000):
        it = C.c_int()
        rel = F64()
        self._ck(self.lib.pgd_bicgstab_solve(self.h, op, b, x, float(rtol), float(atol), int(maxit), C.byref(it), C.byref(rel)))
        return it.value, rel.value

    def band_solve(self, op, b, x):
        self._ck(self.lib.pgd_band_solve(self.h, op, b, x))

    # ---- distributed PCG pieces
    def slots_ptr(self):
        p = VP()
        self._ck(self.lib.pgd_slots_ptr(self.h, C.byref(p)))
        return p.value

    def slots_download(self, first=0, count=NSLOTS):
        out = np.empty(count, dtype=np.float64)
        self._ck(self.lib.pgd_slots_download(self.h, dptr(out), int(first), int(count)))
        return out

    def slots_upload(self, vals, first=0):
        vals = np.ascontiguousarray(vals, dtype=np.float64)
        self._ck(self.lib.pgd_slots_upload(self.h, dptr(vals), int(first), vals.size))

    def flags_reset(self):
        self._ck(self.lib.pgd_flags_reset(self.h))

    def flags(self):
        d, i, s = I32(), I32(), I32()
        self._ck(self.lib.pgd_flags_download(self.h, C.byref(d), C.byref(i), C.byref(s)))
        return d.value, i.value, s.value

    def op_diag_inv(self, op, dinv):
        self._ck(self.lib.pgd_op_diag_inv(self.h, op, dinv))

    def spmv_dot_slot(self, A, x, y, w, r0, r1, slot):
        self._ck(self.lib.pgd_spmv_dot_slot(self.h, A, x, y, w, int(r0), int(r1), int(slot)))

    def pcg_init_slot(self, b, q, dinv, r, z, p, lo, hi, slot):
        self._ck(self.lib.pgd_pcg_init_slot(self.h, b, q, dinv, r, z, p, int(lo), int(hi), int(slot)))

    def pcg_tol_slot(self, rtol, atol, slot_rr, slot_bb, slot_tol2):
        self._ck(self.lib.pgd_pcg_tol_slot(self.h, float(rtol), float(atol), slot_rr, slot_bb, slot_tol2))

    def pcg_xr_slot(self, x, r, p, q, dinv, z, lo, hi, slot_rz, slot_pq, slot_out):
        self._ck(self.lib.pgd_pcg_xr_slot(self.h, x, r, p, q, dinv, z, int(lo), int(hi),
                                          slot_rz, slot_pq, slot_out))

    def pcg_check_slot(self, slot_rr, slot_tol2):
        self._ck(self.lib.pgd_pcg_check_slot(self.h, slot_rr, slot_tol2))

    def pcg_p_slot(self, p, z, lo, hi, slot_num, slot_den):
        self._ck(self.lib.pgd_pcg_p_slot(self.h, p, z, int(lo), int(hi), slot_num, slot_den))

    def cg_init_slot(self, b, q, dinv, r, u, p, s, lo, hi, base):
        self._ck(self.lib.pgd_cg_init_slot(self.h, b, q, dinv, r, u, p, s, int(lo), int(hi), int(base)))

    def cg_update_slot(self, x, r, u, w, p, s, dinv, lo, hi, base):
        self._ck(self.lib.pgd_cg_update_slot(self.h, x, r, u, w, p, s, dinv, int(lo), int(hi), int(base)))

    def cg_scalars_slot(self, base, init, rtol, atol):
        self._ck(self.lib.pgd_cg_scalars_slot(self.h, int(base), int(init), float(rtol), float(atol)))

    # ---- in-library sharded solve
    def comm_bind_callbacks(self, halo, allreduce, rank, world):
        """halo(vec, own0, own1, lo_ghost, hi_ghost), allreduce(first_slot, count): Python callables.  An
        exception inside a callback is kept and re-raised by the library call that triggered it."""
        self._cb_error = None

        def _halo(user, vec, own0, own1, lo_g, hi_g):
            try:
                halo(vec, own0, own1, lo_g, hi_g)
                return 0
            except BaseException as e:      # noqa: BLE001 - must not propagate through the C frame
                self._cb_error = e
                return -1

        def _allreduce(user, first, count):
            try:
                allreduce(first, count)
                return 0
            except BaseException as e:      # noqa: BLE001
                self._cb_error = e
                return -1
        self._cbs = (HALO_FN(_halo), ALLREDUCE_FN(_allreduce))      # keep the thunks alive
        self._ck(self.lib.pgd_comm_bind_callbacks(self.h, self._cbs[0], self._cbs[1], None, int(rank), int(world)))

    def comm_unique_id(self):
        buf = (C.c_uint8 * 128)()
        self._ck(self.lib.pgd_comm_unique_id(self.h, buf))
        return bytes(buf)

    def comm_bind_rccl(self, unique_id, rank, world):
        if len(unique_id) != 128:
            raise ValueError("RCCL unique id must be 128 bytes")
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._ck(self.lib.pgd_comm_bind_rccl(self.h, buf, int(rank), int(world)))

    def comm_overlap(self, mode=-1):
        """mode 1: try to enable the halo/interior overlap (collective), 0: disable, -1: query; returns the state."""
        st = C.c_int(0)
        self._ck(self.lib.pgd_comm_overlap(self.h, int(mode), C.byref(st)))
        return bool(st.value)

    def comm_unbind(self):
        self._ck(self.lib.pgd_comm_unbind(self.h))
        self._cbs = None

    def comm_timeout(self, seconds):
        """Deadline of the host-side waits of the sharded solve (PGD_ERR_TIMEOUT after that long without progress)."""
        self._ck(self.lib.pgd_comm_timeout(self.h, float(seconds)))

    COMM_PHASES = ("samples", "halo_wait", "product_interior", "product_boundary", "local_sums", "allreduce", "update",
                   "host_boundary_wait")

    def comm_prof(self, mode=-1):
        """Phase timing of the sharded loop: mode 1 = on + reset, 0 = off, -1 = read.  Seconds summed over the samples."""
        out = np.zeros(8)
        self._ck(self.lib.pgd_comm_prof(self.h, int(mode), dptr(out)))
        return dict(zip(self.COMM_PHASES, out.tolist()))

    def comm_info(self):
        k, r, w = C.c_int(), C.c_int(), C.c_int()
        self._ck(self.lib.pgd_comm_info(self.h, C.byref(k), C.byref(r), C.byref(w)))
        return {"kind": ("none", "callbacks", "rccl")[k.value], "rank": r.value, "world": w.value}

    def _ck_cb(self, rc):
        err = getattr(self, "_cb_error", None)
        if err is not None:
            self._cb_error = None
            raise err
        self._ck(rc)

    def comm_halo(self, vec, own0, own1, lo_g, hi_g):
        self._ck_cb(self.lib.pgd_comm_halo(self.h, vec, int(own0), int(own1), int(lo_g), int(hi_g)))

    PUSH_BLOB_BYTES = 256

    def comm_push_export(self, n, own0, own1, lo_g, hi_g):
        """Direct halo, step 1: size the sharded loop's work vectors for this partition; returns the blob the neighbours need."""
        buf = (C.c_uint8 * self.PUSH_BLOB_BYTES)()
        self._ck(self.lib.pgd_comm_push_export(self.h, int(n), int(own0), int(own1), int(lo_g), int(hi_g), buf))
        return bytes(buf)

    def comm_push_attach(self, lower, upper):
        """Direct halo, step 2 (collective over the neighbours): the lower / upper neighbour's blob or None.  True if usable here."""
        def arr(b):
            if b is None:
                return None
            if len(b) != self.PUSH_BLOB_BYTES:
                raise ValueError("comm_push_attach: a blob has %d bytes" % self.PUSH_BLOB_BYTES)
            return (C.c_uint8 * self.PUSH_BLOB_BYTES).from_buffer_copy(b)
        st = C.c_int(0)
        self._ck(self.lib.pgd_comm_push_attach(self.h, arr(lower), arr(upper), C.byref(st)))
        return bool(st.value)

    def comm_allreduce_attach(self, blobs):
        """Direct all-reduce (collective over ALL ranks): every rank's export blob in rank order.  True if usable here."""
        data = b"".join(blobs)
        if len(data) != self.PUSH_BLOB_BYTES * len(blobs):
            raise ValueError("comm_allreduce_attach: blobs of %d bytes each" % self.PUSH_BLOB_BYTES)
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        st = C.c_int(0)
        self._ck(self.lib.pgd_comm_allreduce_attach(self.h, buf, C.byref(st)))
        return bool(st.value)

    def comm_allreduce_direct(self, mode=-1):
        st = C.c_int(0)
        self._ck(self.lib.pgd_comm_allreduce_direct(self.h, int(mode), C.byref(st)))
        return bool(st.value)

    def comm_push(self, mode=-1):
        st = C.c_int(0)
        self._ck(self.lib.pgd_comm_push(self.h, int(mode), C.byref(st)))
        return bool(st.value)

    def comm_allreduce_slots(self, first, count):
        self._ck_cb(self.lib.pgd_comm_allreduce_slots(self.h, int(first), int(count)))

    def pcg_solve_sharded(self, op, b, x, own0, own1, lo_g, hi_g, rtol, atol, maxit):
        it, rel = C.c_int(), F64()
        self._ck_cb(self.lib.pgd_pcg_solve_sharded(self.h, op, b, x, int(own0), int(own1), int(lo_g), int(hi_g),
                                                   float(rtol), float(atol), int(maxit), C.byref(it), C.byref(rel)))
        return it.value, rel.value

    def op_symmetrize(self, op):
        used = C.c_int(0)
        self._ck(self.lib.pgd_op_symmetrize(self.h, op, C.byref(used)))
        return bool(used.value)

    def op_classify(self, op):
        """Row-class dictionary of the operator's diagonal form: number of classes, 0 = none (pgd_op_classify)."""
        n = C.c_int(0)
        self._ck(self.lib.pgd_op_classify(self.h, op, C.byref(n)))
        return int(n.value)

    def tune(self, knob, value):
        self._ck(self.lib.pgd_tune(self.h, int(knob), int(value)))
        if int(knob) == TUNE_LOCATE_INDEX:
            self._locate_index = int(value)

    # ---- measuring
    def prof_enable(self, on=True):
        self._ck(self.lib.pgd_prof_enable(self.h, int(on)))

    def prof_read(self):
        n, s, b = I64(), F64(), F64()
        self._ck(self.lib.pgd_prof_read(self.h, C.byref(n), C.byref(s), C.byref(b)))
        own = F64()
        self._ck(self.lib.pgd_prof_read_own(self.h, C.byref(own)))
        un, us, ub = I64(), F64(), F64()
        self._ck(self.lib.pgd_prof_read_update(self.h, C.byref(un), C.byref(us), C.byref(ub)))
        dr, ov = I64(), F64()
        self._ck(self.lib.pgd_prof_read_dropped(self.h, C.byref(dr)))
        self._ck(self.lib.pgd_prof_event_overhead(self.h, C.byref(ov)))
        return dict(launches=n.value, seconds=s.value, bytes=b.value, own_bytes=own.value,
                    update_launches=un.value, update_seconds=us.value, update_bytes=ub.value, dropped_noop_samples=dr.value,
                    event_overhead=ov.value)

    KERNEL_FAMILIES = ("csr", "csr_dict", "sym_rows", "dia_rows", "dia_march", "multi", "diac_march", "stencil_march")

    def kernel_counts(self):
        out = (C.c_int64 * 8)()
        self._ck(self.lib.pgd_kernel_counts(self.h, out, 8))
        return {k: int(out[i]) for i, k in enumerate(self.KERNEL_FAMILIES)}

    def product_plan(self, op, r0=0, r1=-1, pcg_like=True):
        """Kernel family (a name of KERNEL_FAMILIES, None: not decided by form) and launch shape of a product over [r0, r1) of `op`
        as it stands, under the current knobs; launches and counts nothing."""
        out = (C.c_int64 * 7)()
        self._ck(self.lib.pgd_product_plan(self.h, op, int(r0), int(r1), 1 if pcg_like else 0, out, 7))
        plan = dict(zip(("form", "wgs", "zchunk", "tiles_x", "tiles_y", "rows_per_thread", "depth"), map(int, out)))
        plan["family"] = self.KERNEL_FAMILIES[plan["form"]] if plan["form"] >= 0 else None
        return plan

    def pcg_recompute_updates(self):
        """Launches of the PCG update that forms A p itself instead of reading it (PGD_TUNE_PCG_RECOMPUTE_Q)."""
        n = I64()
        self._ck(self.lib.pgd_pcg_recompute_counts(self.h, C.byref(n)))
        return n.value

    def pcg_fused_marches(self):
        """Launches of the march that holds the PCG update and the next product's dots (PGD_TUNE_PCG_FUSED_MARCH)."""
        n = I64()
        self._ck(self.lib.pgd_pcg_fused_counts(self.h, C.byref(n)))
        return n.value

    def classify_counts(self):
        full, cached = I64(), I64()
        self._ck(self.lib.pgd_classify_counts(self.h, C.byref(full), C.byref(cached)))
        return {"full": full.value, "cached": cached.value}

    def _precondition(self, which, stats):
        """PGD_TUNE_PCG_PRECOND = which; the solves that the cycle behind `stats` has preconditioned so far."""
        self.tune(40, which)
        return stats()["solves"]

    def _cycle_stats(self, cycle):
        a, b, l, m, ms = I64(), I64(), I64(), I64(), C.c_double()
        self._ck(getattr(self.lib, "pgd_%s_counts" % cycle)(self.h, C.byref(a), C.byref(b), C.byref(l)))
        self._ck(getattr(self.lib, "pgd_%s_times" % cycle)(self.h, C.byref(ms), C.byref(m)))
        return {"solves": a.value, "fallbacks": b.value, "levels": l.value, "setup_ms": ms.value, "march_passes": m.value}

    def precondition(self, multigrid):
        """Select the preconditioner of the next pcg_solve calls (1: the multigrid V-cycle where the operator allows it,
        0: Jacobi); returns the number of solves the V-cycle has preconditioned so far."""
        return self._precondition(1 if multigrid else 0, self.mg_stats)

    def mg_stats(self):
        a, b = I64(), I64()
        self._ck(self.lib.pgd_mg_counts(self.h, C.byref(a), C.byref(b)))
        return {"solves": a.value, "fallbacks": b.value}

    def precondition_variable(self, on):
        """Select the V-cycle for variable-coefficient operators (PGD_TUNE_PCG_PRECOND = 2) for the next pcg_solve calls, or
        (on false) the Jacobi-PCG again; returns the number of solves that cycle has preconditioned so far."""
        return self._precondition(2 if on else 0, self.vmg_stats)

    def vmg_stats(self):
        return self._cycle_stats("vmg")

    def precondition_component(self, on):
        """Select the component-wise V-cycle for vector-valued P1 operators on box lattices (PGD_TUNE_PCG_PRECOND = 3) for the next
        pcg_solve calls, or (on false) the Jacobi-PCG again; returns the number of solves that cycle has preconditioned so far."""
        return self._precondition(3 if on else 0, self.cmg_stats)

    def cmg_stats(self):
        return self._cycle_stats("cmg")

    def precondition_p(self, on):
        """Select the p-multigrid cycle for P2 operators on bound box lattices (PGD_TUNE_PCG_PRECOND = 4) for the next pcg_solve calls,
        or (on false) the Jacobi-PCG again; returns the number of solves that cycle has preconditioned so far."""
        return self._precondition(4 if on else 0, self.pmg_stats)

    def pmg_stats(self):
        return self._cycle_stats("pmg")

    def pmg_coarse(self, comp, nvert):
        """What the last solve under the p-multigrid cycle built for component comp: (the 8 level-0 slot arrays as an 8 x nvert
        array, the eliminated bytes of the nvert vertices)."""
        slots = np.empty((8, int(nvert)), dtype=np.float64)
        el = np.empty(int(nvert), dtype=np.uint8)
        self._ck(self.lib.pgd_pmg_coarse(self.h, int(comp), dptr(slots), el.ctypes.data_as(PU8)))
        return slots, el

    def _product_form(self, knob, on, stats):
        """Tune knob = on; the products launched so far from the form behind `stats`."""
        self.tune(knob, 1 if on else 0)
        return stats()["products"]

    def _form_stats(self, form):
        f, p, b, ms = I64(), I64(), I64(), C.c_double()
        self._ck(getattr(self.lib, "pgd_%s_counts" % form)(self.h, C.byref(f), C.byref(p), C.byref(b)))
        self._ck(getattr(self.lib, "pgd_%s_times" % form)(self.h, C.byref(ms)))
        return {"forms_built": f.value, "products": p.value, "fallbacks": b.value, "extract_ms": ms.value}

    def block_product(self, on):
        """Select the row-diagonal product for operators on vector-valued P1 layouts over box lattices (PGD_TUNE_SPMV_BLOCK_DIA) for
        the next products and solves, or (on false) the CSR product again; returns the number of products launched from that form
        so far.  The results do not depend on it, bit for bit."""
        return self._product_form(TUNE_SPMV_BLOCK_DIA, on, self.bdia_stats)

    def bdia_stats(self):
        return self._form_stats("bdia")

    def p2_product(self, on):
        """Select the row-class product for operators on P2 layouts bound to 3-D box lattices (PGD_TUNE_SPMV_P2_LATTICE) for the next
        products and solves, or (on false) the CSR product again; returns the number of products launched from that form so far.
        The results do not depend on it, bit for bit."""
        return self._product_form(TUNE_SPMV_P2_LATTICE, on, self.p2lat_stats)

    def p2lat_stats(self):
        return self._form_stats("p2lat")

    def calib_stream(self, v, bytes_per_lane, store=False):
        self._ck(self.lib.pgd_calib_stream(self.h, v, int(bytes_per_lane), int(bool(store))))

    def timer_start(self):
        self._ck(self.lib.pgd_timer_start(self.h))

    def timer_stop(self):
        s = F64()
        self._ck(self.lib.pgd_timer_stop(self.h, C.byref(s)))
        return s.value
