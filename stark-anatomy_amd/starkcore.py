"""ctypes binding of libstarkcore.so (include/starkcore.h) plus the device-resident codeword type.

This is the ONLY path from the host modules (ntt.py, fri.py, merkle.py) to the GPU.  There is no CPU
fallback: if the shared library is missing or no MI355X is visible, calls raise RuntimeError.
"""
import array
import ctypes
import itertools
import os
from collections.abc import Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("STARKCORE_LIB") or os.path.join(_HERE, "libstarkcore.so")   # override only for A/B experiments

_u64 = ctypes.c_uint64
_vp = ctypes.c_void_p
_int = ctypes.c_int

SC_ERR_NOT_POW2 = -2
SC_ERR_ROOT_ORDER = -3
SC_ERR_ROOT_NOT_PRIMITIVE = -4
SC_ERR_DIV_ZERO = -5
SC_ERR_UNSUPPORTED = -7
SC_ERR_TIMEOUT = -9
FOREST_MAX_LEAVES = 1 << 24        # SC_FOREST_MAX_LEAVES of include/starkcore.h: leaves of the largest forest an entry takes

# every symbol include/starkcore.h declares: (restype, argtypes)
SIGNATURES = {
    "sc_device_count": (_int, []),
    "sc_init": (_int, [_int]),
    "sc_shutdown": (_int, []),
    "sc_last_error": (ctypes.c_char_p, []),
    "sc_synchronize": (_int, []),
    "sc_stream": (_int, [ctypes.POINTER(_vp)]),
    "sc_stream_join": (_int, [_vp]),
    "sc_set_tuning": (_int, [ctypes.c_char_p, _int]),
    "sc_ntt_num_passes": (_int, [_u64]),
    "sc_debug_trace": (_int, [_vp]),
    "sc_field_selftest": (_int, [_int, _vp, _vp, _vp, _u64]),
    "sc_field_selftest2": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _vp, _u64]),
    "sc_vec_alloc": (_int, [_u64, ctypes.POINTER(_vp)]),
    "sc_vec_free": (_int, [_vp]),
    "sc_vec_wrap": (_int, [_vp, _u64, ctypes.POINTER(_vp)]),
    "sc_vec_len": (_u64, [_vp]),
    "sc_vec_ptr": (_vp, [_vp]),
    "sc_vec_zero": (_int, [_vp]),
    "sc_vec_upload": (_int, [_vp, _u64, _vp, _u64]),
    "sc_vec_download": (_int, [_vp, _u64, _vp, _u64]),
    "sc_vec_gather": (_int, [_vp, _vp, _u64, _vp]),
    "sc_memcpy_dev": (_int, [_vp, _vp, _u64, _vp]),
    "sc_sample_bytes_dev": (_int, [_vp, _u64, ctypes.c_uint32, _vp, _vp]),
    "sc_randomized_columns_dev": (_int, [_vp, _u64, _u64, _u64, _u64, _vp, _u64, _u64, ctypes.c_uint32, _vp, _u64, _vp]),
    "sc_sample_urandom_dev": (_int, [_u64, ctypes.c_uint32, _vp, _vp]),
    "sc_urandom_prefetch": (_int, [_u64, ctypes.c_uint32]),
    "sc_rescue_prime_hash_dev": (_int, [_vp, _u64, _vp, _u64, _vp, _vp]),
    "sc_rescue_prime_trace_dev": (_int, [_vp, _u64, _vp, _u64, _vp, _vp]),
    "sc_rescue_prime_permute_dev": (_int, [_vp, _u64, _vp, _u64, _u64, _u64, _vp, _u64, _vp]),
    "sc_rescue_prime_sponge_dev": (_int, [_vp, _u64, _u64, _vp, _u64, _u64, _u64, _u64, _u64, _vp, _u64, _vp]),
    "sc_rescue_prime_trace_states_dev": (_int, [_vp, _u64, _u64, _u64, _vp, _u64, _vp, _vp]),
    "sc_rescue_merkle_build_dev": (_int, [_vp, _u64, _u64, _u64, _u64, _u64, _u64, _vp, _u64, _vp, _vp]),
    "sc_rescue_merkle_root": (_int, [_vp, _vp]),
    "sc_rescue_merkle_open_batch": (_int, [_vp, _vp, _u64, _vp]),
    "sc_rescue_merkle_level_copy_dev": (_int, [_vp, _u64, _vp, _vp]),
    "sc_rescue_merkle_verify_batch": (_int, [_vp, _vp, _vp, _vp, _u64, _u64, _u64, _u64, _u64, _u64, _vp, _u64, _vp]),
    "sc_rescue_merkle_path_trace_dev": (_int, [_vp, _vp, _vp, _u64, _u64, _u64, _u64, _u64, _vp, _u64, _vp, _vp]),
    "sc_rescue_merkle_leaves": (_u64, [_vp]),
    "sc_rescue_merkle_free": (_int, [_vp]),
    "sc_grind": (_int, [_vp, _int, _u64, _u64, ctypes.POINTER(_u64), ctypes.POINTER(_int), _vp]),
    "sc_grind_batch": (_int, [_vp, _u64, _int, _u64, _u64, _vp, _vp, _vp]),
    "sc_grind_host": (_int, [_vp, _int, _u64, _u64, ctypes.POINTER(_u64), ctypes.POINTER(_int)]),
    "sc_ntt": (_int, [_vp, _vp, _u64, _vp, _int]),
    "sc_ntt_dev": (_int, [_vp, _vp, _u64, _vp, _int, _vp]),
    "sc_ntt_columns_dev": (_int, [_vp, _vp, _u64, _u64, _vp, _int, _vp]),
    "sc_ntt_batch_dev": (_int, [_vp, _vp, _u64, _u64, _int, _vp, _vp]),
    "sc_ntt_batch_ex_dev": (_int, [_vp, _vp, _u64, _u64, _int, _vp, _vp, _u64, _u64, _int, _u64, _vp]),
    "sc_ntt_rows_t_ld_dev": (_int, [_vp, _vp, _u64, _u64, _vp, _u64, _u64, _vp]),
    "sc_fourstep_create": (_int, [_int, _vp, _int, _int, ctypes.POINTER(_vp)]),
    "sc_fourstep_create_ex": (_int, [_int, _vp, _int, _int, _int, ctypes.POINTER(_vp)]),
    "sc_ipc_region_create": (_int, [_u64, ctypes.POINTER(_vp), _vp]),
    "sc_ipc_region_create_ex": (_int, [_u64, _int, ctypes.POINTER(_vp), _vp]),
    "sc_ipc_region_open": (_int, [_vp, ctypes.POINTER(_vp)]),
    "sc_ipc_region_kind": (_int, [ctypes.POINTER(_int)]),
    "sc_ipc_region_close": (_int, [_vp]),
    "sc_ipc_region_free": (_int, [_vp]),
    "sc_fourstep_region_bytes": (_int, [_vp, ctypes.POINTER(_u64)]),
    "sc_fourstep_set_peers": (_int, [_vp, _vp]),
    "sc_fourstep_run_direct_dev": (_int, [_vp, _int, _vp, _vp, _vp]),
    "sc_fourstep_direct_status": (_int, [_vp, ctypes.POINTER(_u64)]),
    "sc_fourstep_free": (_int, [_vp]),
    "sc_fourstep_shape": (_int, [_vp, _int, ctypes.POINTER(_u64), ctypes.POINTER(_u64)]),
    "sc_fourstep_cols_dev": (_int, [_vp, _int, _vp, _vp, _vp, _vp]),
    "sc_fourstep_rows_dev": (_int, [_vp, _int, _vp, _vp, _u64, _u64, _int, _vp]),
    "sc_fourstep_rows_finish_dev": (_int, [_vp, _int, _vp, _vp]),
    "sc_comm_unique_id": (_int, [ctypes.c_char_p, _vp]),
    "sc_comm_init": (_int, [ctypes.c_char_p, _vp, _int, _int]),
    "sc_comm_destroy": (_int, []),
    "sc_fourstep_run_dev": (_int, [_vp, _int, _vp, _vp, _vp, _vp, _u64, _int, _int, _vp]),
    "sc_twiddle_matrix_dev": (_int, [_vp, _u64, _u64, _u64, _u64, _vp, _u64, _vp, _vp]),
    "sc_coset_evaluate": (_int, [_vp, _u64, _vp, _vp, _u64, _vp]),
    "sc_coset_evaluate_dev": (_int, [_vp, _u64, _vp, _vp, _u64, _vp, _vp]),
    "sc_coset_evaluate_columns_dev": (_int, [_vp, _u64, _u64, _vp, _vp, _u64, _vp, _vp]),
    "sc_poly_mul": (_int, [_vp, _u64, _vp, _u64, _vp, _u64, _vp, _u64]),
    "sc_coset_divide": (_int, [_vp, _u64, _vp, _u64, _vp, _vp, _u64, _vp, _u64]),
    "sc_coset_divide_dev": (_int, [_vp, _u64, _vp, _u64, _vp, _vp, _u64, _vp, _u64, ctypes.POINTER(_int), _vp]),
    "sc_vec_degree_dev": (_int, [_vp, _u64, ctypes.POINTER(ctypes.c_int64), _vp]),
    "sc_vec_degree_columns_dev": (_int, [_vp, _u64, _u64, _u64, ctypes.POINTER(ctypes.c_int64), _vp]),
    "sc_pointwise_mul_dev": (_int, [_vp, _vp, _vp, _u64, _vp]),
    "sc_pointwise_div_dev": (_int, [_vp, _vp, _vp, _u64, _vp]),
    "sc_poly_mul_dev": (_int, [_vp, _u64, _vp, _u64, _vp, _vp]),
    "sc_poly_mul_columns_dev": (_int, [_vp, _u64, _u64, _u64, _vp, _u64, _u64, _vp, _u64, _vp]),
    "sc_poly_pow_dev": (_int, [_vp, _u64, _u64, _vp, _vp]),
    "sc_poly_product_dev": (_int, [_vp, _u64, _u64, _u64, _vp, _vp]),
    "sc_poly_eval_points_dev": (_int, [_vp, _u64, _u64, _u64, _vp, _u64, _vp, _u64, _vp]),
    "sc_poly_eval_points": (_int, [_vp, _u64, _vp, _u64, _vp]),
    "sc_poly_divmod": (_int, [_vp, _u64, _vp, _u64, _vp, _vp]),
    "sc_poly_divmod_dev": (_int, [_vp, _u64, _vp, _u64, _vp, _vp, _vp]),
    "sc_poly_divmod_columns_dev": (_int, [_vp, _u64, _u64, _u64, _vp, _u64, _vp, _u64, _vp, _u64, _vp]),
    "sc_coset_divide_later_dev": (_int, [_vp, _u64, _vp, _u64, _vp, _vp, _u64, _vp, _u64, ctypes.POINTER(_vp), _vp]),
    "sc_pointwise_div_later_dev": (_int, [_vp, _vp, _vp, _u64, ctypes.POINTER(_vp), _vp]),
    "sc_later_wait": (_int, [_vp, ctypes.POINTER(ctypes.c_int64)]),
    "sc_pointwise_div_columns_later_dev": (_int, [_vp, _u64, _vp, _u64, _vp, _u64, _u64, _u64, ctypes.POINTER(_vp), _vp]),
    "sc_coset_divide_columns_later_dev": (_int, [_vp, _u64, _u64, _vp, _u64, _u64, _u64, _vp, _vp, _u64, _vp, ctypes.POINTER(_u64), _u64, ctypes.POINTER(_vp), _vp]),
    "sc_combine_columns_dev": (_int, [_vp, _u64, _vp, _u64, _vp, _u64, _u64, _vp]),
    "sc_scale_dev": (_int, [_vp, _vp, _u64, _vp, _vp]),
    "sc_scale_columns_dev": (_int, [_vp, _u64, _vp, _u64, _u64, _u64, _vp, _vp]),
    "sc_axpy_shift_dev": (_int, [_vp, _u64, _vp, _u64, _u64, _vp, _vp]),
    "sc_scale_slab_dev": (_int, [_vp, _vp, _u64, _u64, _u64, _u64, _vp, _vp]),
    "sc_fri_fold": (_int, [_vp, _u64, _vp, _vp, _vp, _vp]),
    "sc_fri_fold_dev": (_int, [_vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "sc_merkle_commit": (_int, [_vp, _u64, _vp]),
    "sc_merkle_build": (_int, [_vp, _u64, _vp, ctypes.POINTER(_vp)]),
    "sc_merkle_build_dev": (_int, [_vp, _u64, _vp, ctypes.POINTER(_vp), _vp]),
    "sc_merkle_build_async_dev": (_int, [_vp, _u64, ctypes.POINTER(_vp), _vp]),
    "sc_merkle_build_noroot_dev": (_int, [_vp, _u64, ctypes.POINTER(_vp), _vp]),
    "sc_merkle_root": (_int, [_vp, _vp]),
    "sc_fri_fold_commit_dev": (_int, [_vp, _u64, _vp, _vp, _vp, _vp, ctypes.POINTER(_vp), _vp]),
    "sc_fri_commit_dev": (_int, [_vp, _u64, _vp, _vp, ctypes.c_uint32, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "sc_fri_prove_dev": (_int, [_vp, _u64, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp,
                                _vp, _vp, _vp, _vp, _u64, _vp]),
    "sc_fri_prove_grind_dev": (_int, [_vp, _u64, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp,
                                      _vp, _vp, _vp, _vp, _u64, _vp, _int, ctypes.POINTER(_u64)]),
    "sc_fri_tail_stats": (_int, [_vp]),
    "sc_host_alloc": (_int, [_u64, _vp]),
    "sc_host_free": (_int, [_vp]),
    "sc_shake256": (_int, [_vp, _u64, _vp, _u64]),
    "sc_pickle_proof": (_int, [_vp, _u64, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp, _u64, ctypes.POINTER(_u64)]),
    "sc_field_sample": (_int, [_vp, _u64, _vp]),
    "sc_blake2b": (_int, [_vp, _u64, _vp]),
    "sc_transcript_challenge": (_int, [_vp, _vp, _u64, _vp, _vp, _u64]),
    "sc_fri_sample_indices": (_int, [_vp, _u64, _u64, _u64, ctypes.c_uint32, _vp]),
    "sc_transcript_bytes": (_int, [_vp, _vp, _u64, _vp, _u64, ctypes.POINTER(_u64)]),
    "sc_merkle_open": (_int, [_vp, _u64, _vp]),
    "sc_merkle_open_batch": (_int, [_vp, _vp, _u64, _vp]),
    "sc_merkle_verify_batch": (_int, [_vp, _u64, _vp, _u64, _vp, _u64, _vp]),
    "sc_fri_colinearity_batch": (_int, [_vp, _u64, _vp, _u64, _vp]),
    "sc_stark_combination_batch": (_int, [_vp, _vp, _u64, _vp]),
    "sc_merkle_query_dev": (_int, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "sc_merkle_query_multi_dev": (_int, [_u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_merkle_level_copy_dev": (_int, [_vp, _int, _vp, _vp]),
    "sc_merkle_from_digests_dev": (_int, [_vp, _u64, _vp, ctypes.POINTER(_vp), _vp]),
    "sc_fri_fold_slab_dev": (_int, [_vp, _u64, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _vp]),
    "sc_fri_fold_slab_build_dev": (_int, [_vp, _u64, _u64, _u64, _u64, _vp, _vp, _vp, _vp, ctypes.POINTER(_vp), _vp]),
    "sc_merkle_leaves": (_u64, [_vp]),
    "sc_merkle_free": (_int, [_vp]),
    "sc_merkle_rows_build_dev": (_int, [_vp, _u64, _u64, _vp, ctypes.POINTER(_vp), _vp]),
    "sc_merkle_rows_build_async_dev": (_int, [_vp, _u64, _u64, ctypes.POINTER(_vp), _vp]),
    "sc_merkle_rows_query_dev": (_int, [_vp, _vp, _u64, _vp, _u64, _vp, _vp]),
    "sc_merkle_row_leaf": (_int, [_vp, _u64, _vp]),
    "sc_fri_fold_pairs_commit_dev": (_int, [_vp, _u64, _vp, _vp, _vp, _vp, ctypes.POINTER(_vp), _vp]),
    "sc_fri_pairs_query_dev": (_int, [_u64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_fri_prove_pairs_dev": (_int, [_vp, _u64, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp,
                                      _vp, _vp, _vp, _vp, _u64, _vp, _int, ctypes.POINTER(_u64)]),
    "sc_merkle_forest_build_dev": (_int, [_vp, _u64, _u64, ctypes.POINTER(_vp), _vp]),
    "sc_fri_fold_forest_dev": (_int, [_vp, _u64, _u64, _vp, _vp, _vp, _vp, ctypes.POINTER(_vp), _vp]),
    "sc_merkle_forest_roots": (_int, [_vp, _vp]),
    "sc_merkle_forest_trees": (_u64, [_vp]),
    "sc_merkle_forest_leaves": (_u64, [_vp]),
    "sc_merkle_forest_free": (_int, [_vp]),
    "sc_merkle_forest_query_dev": (_int, [_u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sc_merkle_forest_stats": (_int, [_vp]),
    "sc_merkle_row_forest_build_dev": (_int, [_vp, _u64, _u64, _u64, ctypes.POINTER(_vp), _vp]),
    "sc_merkle_row_forest_query_dev": (_int, [_vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp]),
    "sc_mpoly_eval_dev": (_int, [_vp, _u64, _u64, _vp, _vp, _u64, _vp, _vp]),
    "sc_mpoly_eval_ex_dev": (_int, [_vp, _u64, _u64, _vp, _vp, _u64, _vp, _int, _vp]),
    "sc_mpoly_eval_rot_dev": (_int, [_vp, _u64, _u64, _vp, _vp, _u64, _vp, _int, _vp, _vp, _vp]),
    "sc_mpoly_eval_columns_dev": (_int, [_vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _vp]),
    "sc_zerofier": (_int, [_vp, _u64, _vp]),
    "sc_evaluate": (_int, [_vp, _u64, _vp, _u64, _vp]),
    "sc_interpolate": (_int, [_vp, _vp, _u64, _vp]),
    "sc_polytree_build": (_int, [_vp, _u64, ctypes.POINTER(_vp)]),
    "sc_polytree_build_dev": (_int, [_vp, _u64, ctypes.POINTER(_vp), _vp]),
    "sc_polytree_points": (_u64, [_vp]),
    "sc_polytree_zerofier_dev": (_int, [_vp, _vp, _vp]),
    "sc_polytree_evaluate_dev": (_int, [_vp, _vp, _u64, _vp, _vp, _vp]),
    "sc_polytree_interpolate_dev": (_int, [_vp, _vp, _vp, _vp]),
    "sc_polytree_evaluate_columns_dev": (_int, [_vp, _vp, _u64, _u64, _u64, _vp, _vp, _u64, _vp]),
    "sc_polytree_interpolate_columns_dev": (_int, [_vp, _vp, _u64, _u64, _vp, _u64, _vp]),
    "sc_polytree_interpolate_lagrange_columns_dev": (_int, [_vp, _vp, _u64, _u64, _vp, _u64, _vp]),
    "sc_interpolate_lagrange": (_int, [_vp, _vp, _u64, _vp]),
    "sc_polytree_free": (_int, [_vp]),
    "sc_geodomain_create": (_int, [_vp, _vp, _u64, ctypes.POINTER(_vp), _vp]),
    "sc_geodomain_points": (_u64, [_vp]),
    "sc_geodomain_detect_dev": (_int, [_vp, _u64, _vp, _vp, ctypes.POINTER(_int), _vp]),
    "sc_geodomain_zerofier_dev": (_int, [_vp, _vp, _vp]),
    "sc_geodomain_evaluate_dev": (_int, [_vp, _vp, _u64, _vp, _vp]),
    "sc_geodomain_interpolate_dev": (_int, [_vp, _vp, _vp, _vp]),
    "sc_geodomain_interpolate_columns_dev": (_int, [_vp, _vp, _u64, _u64, _vp, _u64, _vp]),
    "sc_geodomain_evaluate_columns_dev": (_int, [_vp, _vp, _u64, _u64, _u64, _vp, _u64, _vp]),
    "sc_geodomain_free": (_int, [_vp]),
}

_lib = None


def _one_hip_runtime():
    """torch wheels carry their own copy of the HIP runtime (same soname as /opt/rocm's).  Two copies in one process do not share
    the device: if libstarkcore.so pulled in the system copy first, a later `import torch` would find "No HIP GPUs".  When torch is
    installed but not imported yet, its copy of libamdhip64 is therefore loaded (by path, RTLD_GLOBAL) before the library, so
    that libstarkcore's DT_NEEDED binds to it by soname and a later `import torch` (sharded.py and bench.py use torch for memory,
    streams and collectives in the same process) finds the same runtime -- without importing torch here: a pure C-ABI user pays
    milliseconds, not the seconds and side effects of the import.  Only if that preload fails torch itself is imported; a failure
    of both is reported, not hidden.  STARKCORE_NO_TORCH=1 skips all of it (a process that never touches torch)."""
    import importlib.util
    import sys
    import warnings
    if "torch" in sys.modules or os.environ.get("STARKCORE_NO_TORCH") == "1":
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    runtime = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    try:
        if os.path.exists(runtime):
            ctypes.CDLL(runtime, mode=ctypes.RTLD_GLOBAL)
            return
    except OSError as e:
        warnings.warn("starkcore: could not preload torch's HIP runtime (%s); importing torch instead" % e)
    try:
        import torch  # noqa: F401
    except Exception as e:      # noqa: BLE001  a broken torch install must not take the library down with it -- but say so
        warnings.warn("starkcore: torch is installed but neither its HIP runtime nor torch itself could be loaded (%r); a later "
                      "`import torch` in this process may not see the GPU (set STARKCORE_NO_TORCH=1 to silence)" % (e,))


def lib():
    """The loaded library (loads on first use; raises if the HIP extension was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError("libstarkcore.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "or `make -C stark-anatomy_amd/csrc` (the HIP extension is mandatory, there is no CPU fallback)")
        _one_hip_runtime()
        l = ctypes.CDLL(_LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


class StarkCoreError(RuntimeError):
    pass


def _check(rc):
    """Map a negative return code to the exception the reference's `assert` would have raised."""
    if rc == 0:
        return
    msg = lib().sc_last_error().decode(errors="replace")
    if rc in (SC_ERR_NOT_POW2, SC_ERR_ROOT_ORDER, SC_ERR_ROOT_NOT_PRIMITIVE, SC_ERR_DIV_ZERO):
        raise AssertionError(msg)
    raise StarkCoreError("starkcore error %d: %s" % (rc, msg))


def device_count():
    return lib().sc_device_count()


def init(device=-1):
    _check(lib().sc_init(device))


def set_tuning(key, value):
    _check(lib().sc_set_tuning(key.encode(), int(value)))


def synchronize():
    _check(lib().sc_synchronize())


def library_stream():
    """the library's own HIP stream as an integer handle (for torch.cuda.ExternalStream: work put on it needs no ordering with
    the library's)"""
    h = _vp()
    _check(lib().sc_stream(ctypes.byref(h)))
    return int(h.value or 0)


def stream_join(other):
    """order the library stream and the raw stream handle `other` with each other on the device; the host does not wait"""
    _check(lib().sc_stream_join(_vp(int(other))))


def pickle_proof(ops, moduli, nfields, modulus_bytes, expect=0):
    """pickle.dumps of the object graph described by `ops` (csrc/proof_pickle.h; host only).  expect: bytes of payload the
    description refers to by address (they appear in the output, not in `ops`)"""
    import numpy as np
    need = ctypes.c_uint64()
    size = len(ops) + int(expect)
    cap = size + size // 8 + 4096
    # one scratch buffer per THREAD (the library call releases the GIL), grown when a proof needs more: fresh megabytes from the
    # allocator are page faults on first touch (a 3 MB proof: more time than pickling it), a zeroed ctypes buffer a memset on top
    out = getattr(_pickle_scratch, "buffer", None)
    if out is None or out.size < cap:
        out = _pickle_scratch.buffer = np.empty(cap + cap // 4, dtype=np.uint8)
    _check(lib().sc_pickle_proof(ops, len(ops), moduli, nfields, modulus_bytes, _vp(out.ctypes.data), out.size, ctypes.byref(need)))
    if need.value > out.size:
        out = _pickle_scratch.buffer = np.empty(need.value + need.value // 4, dtype=np.uint8)
        _check(lib().sc_pickle_proof(ops, len(ops), moduli, nfields, modulus_bytes, _vp(out.ctypes.data), out.size, ctypes.byref(need)))
    return out[:need.value].tobytes()


import threading as _threading
_pickle_scratch = _threading.local()


def fe_bytes(v):
    """int residue -> 16 little-endian bytes (the ABI's element layout)."""
    return int(v).to_bytes(16, "little")


def pack(values):
    """iterable of ints -> packed bytes (one C-level pass: int.to_bytes mapped over the values; anything that is not an int --
    numpy scalars, for instance -- goes through int() first)."""
    values = values if isinstance(values, (list, tuple)) else list(values)
    try:
        return b"".join(map(int.to_bytes, values, itertools.repeat(16), itertools.repeat("little")))
    except TypeError:
        return b"".join(int(v).to_bytes(16, "little") for v in values)


def unpack(buf, count=None):
    """packed elements -> Python ints (one C-level pass over the limbs, then lo | hi << 64)"""
    if count is None:
        count = len(buf) // 16
    limbs = _limb_struct(count).unpack_from(buf)
    return [lo | (hi << 64) for lo, hi in zip(limbs[0::2], limbs[1::2])]


_limb_structs = {}


def _limb_struct(count):
    import struct
    st = _limb_structs.get(count)
    if st is None:
        if len(_limb_structs) > 64:
            _limb_structs.clear()
        st = _limb_structs[count] = struct.Struct("<%dQ" % (2 * count))
    return st


# ------------------------------------------------------------------------------------------------
class DeviceVector:
    """Owner of an sc_vec_t (device-resident field elements)."""

    def __init__(self, n):
        self.n = int(n)
        h = _vp()
        _check(lib().sc_vec_alloc(self.n, ctypes.byref(h)))
        self._h = h

    @classmethod
    def wrap(cls, ptr, n, keep):
        """a vector over device memory somebody else owns (sc_vec_wrap): `keep` -- the owner, e.g. a torch tensor -- stays alive
        as long as this object does.  No copy."""
        v = cls.__new__(cls)
        v.n = int(n)
        h = _vp()
        _check(lib().sc_vec_wrap(_vp(int(ptr)), v.n, ctypes.byref(h)))
        v._h, v._keep = h, keep
        return v

    @property
    def __cuda_array_interface__(self):
        """the elements as an [n][2] array of int64 limbs for whoever speaks the CUDA array interface (torch.as_tensor(vec,
        device=...) is a view: no copy; the consumer keeps this object alive)"""
        return {"shape": (self.n, 2), "typestr": "<i8", "data": (int(self.ptr), False), "version": 3, "strides": None}

    @classmethod
    def adopt(cls, handle, n):
        """owner of an sc_vec_t the library handed out (sc_fri_commit_dev's folded codewords)"""
        v = cls.__new__(cls)
        v.n = int(n)
        v._h = _vp(handle) if not isinstance(handle, _vp) else handle
        return v

    @classmethod
    def from_bytes(cls, data):
        v = cls(len(data) // 16)
        if v.n:
            _check(lib().sc_vec_upload(v._h, 0, bytes(data), v.n))
        return v

    @classmethod
    def from_ints(cls, values):
        return cls.from_bytes(pack(values))

    @classmethod
    def zeros(cls, n):
        v = cls(n)
        _check(lib().sc_vec_zero(v._h))
        return v

    def axpy_shift(self, src, shift, weight):
        """self[shift + j] += weight * src[j]  (one term of the nonlinear combination, code/fast_stark.py:130-145)"""
        _check(lib().sc_axpy_shift_dev(self.ptr, self.n, src.ptr, src.n, int(shift), fe_bytes(weight), None))

    @property
    def ptr(self):
        return lib().sc_vec_ptr(self._h)

    def to_bytes(self, offset=0, count=None):
        count = self.n - offset if count is None else count
        out = ctypes.create_string_buffer(16 * count if count else 16)
        if count:
            _check(lib().sc_vec_download(self._h, offset, out, count))
        return out.raw[:16 * count]

    def gather(self, indices):
        k = len(indices)
        if k == 0:
            return []
        idx = (ctypes.c_uint64 * k)(*[int(i) for i in indices])
        out = ctypes.create_string_buffer(16 * k)
        _check(lib().sc_vec_gather(self._h, idx, k, out))
        return unpack(out.raw, k)

    def free(self):
        if self._h is not None and _lib is not None:
            _lib.sc_vec_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _HostMemory:
    """one sc_host_alloc'ed block; goes back to the library's pool when the last reference dies"""

    def __init__(self, nbytes):
        p = _vp()
        _check(lib().sc_host_alloc(max(int(nbytes), 1), ctypes.byref(p)))
        self.ptr = p

    def __del__(self):
        p, self.ptr = getattr(self, "ptr", None), None
        if p is not None and _lib is not None:
            _lib.sc_host_free(p)


class CombineTerm(ctypes.Structure):
    """sc_combine_term_t: one term of sc_combine_columns_dev -- column c of the source at element c * ld, n coefficients, shifted up by `shift`"""
    _fields_ = [("d_src", ctypes.c_void_p), ("ld", ctypes.c_uint64), ("n", ctypes.c_uint64), ("shift", ctypes.c_uint64)]


class Later:
    """A check that is read later (include/starkcore.h sc_later_t): the flags of a division enqueued with sc_*_later_dev.  `wait()`
    -> (a divisor value was zero, the division left a remainder), once; a handle nobody waited for is collected when it is dropped."""

    def __init__(self, handle):
        self._h = handle

    def wait(self):
        words = (ctypes.c_int64 * 8)()
        h, self._h = self._h, None
        _check(lib().sc_later_wait(h, words))
        return words[0] != 0, words[1] >= 0

    def __del__(self):
        if getattr(self, "_h", None) is not None:
            try:
                words = (ctypes.c_int64 * 8)()
                lib().sc_later_wait(self._h, words)
            except Exception:      # noqa: BLE001  (interpreter shutdown)
                pass
            self._h = None


class HostBuffer:
    """Pinned, device-visible host memory from the library's pool (sc_host_alloc): what sc_fri_prove_dev's query kernel writes a
    proof's openings to.  `array` is a uint8 numpy view; views of it keep the memory alive, and it goes back to the pool when the
    last of them dies -- by reference counting (array -> ctypes block -> _HostMemory, no cycle): a block that waited for the cycle
    collector would make the next proof allocate a fresh one (hipHostMalloc of megabytes: 0.1 ms)."""

    def __init__(self, nbytes):
        import numpy as np
        self.nbytes = int(nbytes)
        memory = _HostMemory(self.nbytes)
        self.ptr = memory.ptr
        raw = (ctypes.c_uint8 * max(self.nbytes, 1)).from_address(memory.ptr.value)
        raw._memory = memory                                # numpy keeps `raw` as the array's base; `raw` keeps the block
        self.array = np.frombuffer(raw, dtype=np.uint8, count=self.nbytes)


def query_codewords(codewords, requests):
    """DeviceCodeword.query for several codewords in ONE device round trip: requests[t] = indices into codewords[t];
    returns [(entries, paths)] in the same order (entries identity-preserving, paths fresh objects)."""
    n = len(codewords)
    trees = [cw.tree() for cw in codewords]
    try:
        flat = array.array("Q", itertools.chain.from_iterable(requests))  # (the upper bound is checked by the library)
    except OverflowError:
        raise AssertionError("cannot open invalid index")
    total = len(flat)
    if total == 0:
        return [([], []) for _ in codewords]
    depths = [t.depth for t in trees]
    path_bytes = sum(64 * d * len(req) for d, req in zip(depths, requests))
    elems = ctypes.create_string_buffer(16 * total)
    paths = ctypes.create_string_buffer(path_bytes if path_bytes else 64)
    _check(lib().sc_merkle_query_multi_dev(n, (_vp * n)(*[t._h for t in trees]), (_vp * n)(*[cw.vec.ptr for cw in codewords]),
                                           (ctypes.c_uint64 * total).from_buffer(flat), (ctypes.c_uint64 * n)(*[len(req) for req in requests]), elems, paths))
    values = unpack(elems.raw, total)
    view = memoryview(paths)
    out, vo, po = [], 0, 0
    for cw, req, d in zip(codewords, requests, depths):
        k = len(req)
        out.append((cw._entries(req, values[vo:vo + k]), _path_lists(view, po, d, k)))
        vo += k
        po += 64 * k * d
    return out


# The batched verifier's rows (csrc/merkle_verify.cuh MerkleCheckRow / ColinearityRow / ColinearityRound; include/starkcore.h)
def _row_dtypes():
    import numpy as np
    merkle = np.dtype([("position", "<u8"), ("path", "<u8"), ("root", "<u4"), ("depth", "<u4"), ("kind", "<u4"), ("reserved", "<u4"),
                       ("leaf", "<u8", (2,))])
    colinearity = np.dtype([("a", "<u8"), ("b", "<u8"), ("round", "<u4"), ("reserved", "<u4", (3,)), ("ya", "<u8", (2,)), ("yb", "<u8", (2,)),
                            ("yc", "<u8", (2,))])
    rnd = np.dtype([("offset", "<u8", (2,)), ("omega", "<u8", (2,)), ("alpha", "<u8", (2,))])
    assert (merkle.itemsize, colinearity.itemsize, rnd.itemsize) == (48, 80, 48)
    return merkle, colinearity, rnd


MERKLE_ROW, COLINEARITY_ROW, COLINEARITY_ROUND = _row_dtypes()
LEAF_RESIDUE, LEAF_DIGEST = 0, 1
UNDECIDED = 2


def merkle_rows(positions, paths, roots, depths, kinds, leaves):
    """a MERKLE_ROW array from columns; leaves: 16 bytes per row (the residue little-endian, or the leaf digest's index)"""
    import numpy as np
    rows = np.zeros(len(positions), dtype=MERKLE_ROW)
    if len(rows):
        rows["position"], rows["path"], rows["root"], rows["depth"], rows["kind"] = positions, paths, roots, depths, kinds
        rows["leaf"] = np.frombuffer(leaves, dtype="<u8").reshape(len(rows), 2)
    return rows


def colinearity_rows(a, b, rounds, ys):
    """a COLINEARITY_ROW array from columns; ys: 48 bytes per row (y_a, y_b, y_c, 16 bytes little-endian each)"""
    import numpy as np
    rows = np.zeros(len(a), dtype=COLINEARITY_ROW)
    if len(rows):
        rows["a"], rows["b"], rows["round"] = a, b, rounds
        y = np.frombuffer(ys, dtype="<u8").reshape(len(rows), 6)
        rows["ya"], rows["yb"], rows["yc"] = y[:, 0:2], y[:, 2:4], y[:, 4:6]
    return rows


def merkle_verify_batch(rows, digests, roots):
    """sc_merkle_verify_batch: rows (a MERKLE_ROW array), digests and roots (bytes, 64 per entry) -> uint8 verdicts (1 = the path
    leads to the root)"""
    import numpy as np
    rows = np.ascontiguousarray(rows, dtype=MERKLE_ROW)
    out = np.zeros(len(rows), dtype=np.uint8)
    if len(rows):
        _check(lib().sc_merkle_verify_batch(rows.ctypes.data, len(rows), digests, len(digests) // 64, roots, len(roots) // 64, out.ctypes.data))
    return out


def colinearity_batch(rows, rounds):
    """sc_fri_colinearity_batch: rows (a COLINEARITY_ROW array) over rounds (a COLINEARITY_ROUND array, or 48 bytes each) -> uint8 verdicts
    (1 / 0, UNDECIDED: the caller decides the row with test_colinearity)"""
    import numpy as np
    rows = np.ascontiguousarray(rows, dtype=COLINEARITY_ROW)
    rounds = np.frombuffer(rounds, dtype=COLINEARITY_ROUND) if isinstance(rounds, bytes) else np.ascontiguousarray(rounds, dtype=COLINEARITY_ROUND)
    out = np.zeros(len(rows), dtype=np.uint8)
    if len(rows):
        _check(lib().sc_fri_colinearity_batch(rows.ctypes.data, len(rows), rounds.ctypes.data, len(rounds), out.ctypes.data))
    return out


class _CombinationShared(ctypes.Structure):
    """sc_combination_t of include/starkcore.h"""
    _fields_ = [("registers", _u64), ("ncons", _u64), ("nterms", _vp), ("exps", _vp), ("coefs", _vp), ("generator", _u64 * 2), ("omega", _u64 * 2),
                ("domain_length", _u64), ("step", _u64), ("transition_shifts", _vp), ("boundary_shifts", _vp), ("members", _u64), ("weights", _vp),
                ("polys", _vp), ("pool", _vp), ("pool_len", _u64)]


def combination_row_dtype(registers):
    """a row of sc_stark_combination_batch for an AIR of `registers` registers (csrc/combination.cuh CombRowHead and its leaves)"""
    import numpy as np
    row = np.dtype([("member", "<u8"), ("index", "<u8"), ("claimed", "<u8", (2,)), ("randomizer", "<u8", (2,)), ("zerofier", "<u8", (2,)),
                    ("current", "<u8", (registers, 2)), ("next", "<u8", (registers, 2))])
    assert row.itemsize == 64 + 32 * registers
    return row


class Combination:
    """What the rows of one sc_stark_combination_batch call share, as the C structure and the buffers it points into.  nterms: terms per
    constraint; exps: their [terms][1 + 2 registers] exponent bytes; coefs, weights, pool: packed residues (16 bytes little-endian);
    polys: per member and register (zerofier offset, length, interpolant offset, length) in elements of the pool."""

    def __init__(self, registers, nterms, exps, coefs, generator, omega, domain_length, step, transition_shifts, boundary_shifts, members, weights, polys, pool):
        import numpy as np
        ncons = len(nterms)
        # 16-byte elements in numpy arrays of their own: aligned, and alive as long as this object
        as_words = lambda raw: np.frombuffer(bytes(raw), dtype="<u8").copy() if len(raw) else np.zeros(2, dtype="<u8")
        self._keep = [np.asarray(list(nterms) or [0], dtype="<u8"), np.frombuffer(bytes(exps) or b"\0", dtype=np.uint8).copy(), as_words(coefs),
                      np.asarray(list(transition_shifts) or [0], dtype="<u8"), np.asarray(list(boundary_shifts), dtype="<u8"), as_words(weights),
                      np.ascontiguousarray(polys, dtype="<u8").reshape(-1), as_words(pool)]
        at = [a.ctypes.data for a in self._keep]
        self.registers = registers
        self.struct = _CombinationShared(registers, ncons, at[0], at[1], at[2], (_u64 * 2)(*fe_words(generator)), (_u64 * 2)(*fe_words(omega)), domain_length, step,
                                         at[3], at[4], members, at[5], at[6], at[7], len(pool) // 16)


def fe_words(value):
    return value & 0xFFFFFFFFFFFFFFFF, value >> 64


def combination_batch(shared, rows):
    """sc_stark_combination_batch: rows (an array of combination_row_dtype(shared.registers)) over a Combination -> uint8 verdicts (1 / 0,
    UNDECIDED: the caller decides the row with the host loop)"""
    import numpy as np
    rows = np.ascontiguousarray(rows, dtype=combination_row_dtype(shared.registers))
    out = np.zeros(len(rows), dtype=np.uint8)
    if len(rows):
        _check(lib().sc_stark_combination_batch(ctypes.byref(shared.struct), rows.ctypes.data, len(rows), out.ctypes.data))
    return out


def query_pairs(codewords, requests):
    """The query phase of a proof with pair leaves (Fri(pair_leaves=True), csrc/fri_pairs.cuh) in ONE device round trip: requests[t] =
    leaf numbers a < len(codewords[t]) / 2 of codewords[t]'s pair tree; returns [(pairs, paths)] in the same order -- pairs[i] =
    (cw[a], cw[a + half]) as identity-preserving entries, paths[i] the fresh digests of leaf a's path.  The kernel writes into pinned
    memory of the library's pool."""
    n = len(codewords)
    trees = [cw.pair_tree() for cw in codewords]
    try:
        flat = array.array("Q", itertools.chain.from_iterable(requests))  # (the upper bound is checked by the library)
    except OverflowError:
        raise AssertionError("cannot open invalid index")
    total = len(flat)
    if total == 0:
        return [([], []) for _ in codewords]
    depths = [t.depth for t in trees]
    pair_bytes = (32 * total + 255) & ~255
    path_bytes = sum(64 * d * len(req) for d, req in zip(depths, requests))
    out = HostBuffer(pair_bytes + max(path_bytes, 64))
    _check(lib().sc_fri_pairs_query_dev(n, (_vp * n)(*[t._h for t in trees]), (_vp * n)(*[cw.vec.ptr for cw in codewords]),
                                        (ctypes.c_uint64 * total).from_buffer(flat), (ctypes.c_uint64 * n)(*[len(req) for req in requests]),
                                        out.ptr, _vp(out.ptr.value + pair_bytes)))
    values = unpack(out.array[:32 * total].tobytes(), 2 * total)
    view = memoryview(out.array[pair_bytes:pair_bytes + path_bytes].tobytes())
    answers, vo, po = [], 0, 0
    for cw, req, d in zip(codewords, requests, depths):
        k, half = len(req), cw.vec.n // 2
        mine = values[2 * vo:2 * (vo + k)]
        entries = cw._entries(list(req) + [a + half for a in req], mine[0::2] + mine[1::2])
        answers.append((list(zip(entries[:k], entries[k:])), _path_lists(view, po, d, k)))
        vo += k
        po += 64 * k * d
    return answers


def query_codewords_raw(codewords, requests):
    """query_codewords without objects: [(packed residues (bytes, 16 per opening), paths as a uint8 array [openings][64 * depth])]
    -- what proof_objects' segments keep until somebody asks for the objects"""
    import numpy as np
    n = len(codewords)
    trees = [cw.tree() for cw in codewords]
    try:
        flat = array.array("Q", itertools.chain.from_iterable(requests))
    except OverflowError:
        raise AssertionError("cannot open invalid index")
    total = len(flat)
    if total == 0:
        return [(b"", np.zeros((0, 64 * t.depth), dtype=np.uint8)) for t in trees]
    depths = [t.depth for t in trees]
    path_bytes = sum(64 * d * len(req) for d, req in zip(depths, requests))
    elems = np.empty(16 * total, dtype=np.uint8)                  # (uninitialised: the library fills every byte it is asked for;
    raw_p = np.empty(path_bytes if path_bytes else 64, dtype=np.uint8)   # a zeroed ctypes buffer of megabytes is a memset for nothing)
    _check(lib().sc_merkle_query_multi_dev(n, (_vp * n)(*[t._h for t in trees]), (_vp * n)(*[cw.vec.ptr for cw in codewords]),
                                           (ctypes.c_uint64 * total).from_buffer(flat), (ctypes.c_uint64 * n)(*[len(req) for req in requests]),
                                           _vp(elems.ctypes.data), _vp(raw_p.ctypes.data)))
    raw_e = elems.tobytes()
    out, vo, po = [], 0, 0
    for req, d in zip(requests, depths):
        k = len(req)
        out.append((raw_e[16 * vo:16 * (vo + k)], raw_p[po:po + 64 * k * d].reshape(k, 64 * d)))
        vo += k
        po += 64 * k * d
    return out


class PolyTree:
    """Owner of an sc_polytree_t: the subproduct tree over a list of points, resident in HBM (code/ntt.py:66-130).

    One tree serves the zerofier, any number of multipoint evaluations and interpolations over the same points."""

    def __init__(self, points):
        """points: DeviceVector or packed bytes (16 bytes per point), at least one point"""
        self.points = points if isinstance(points, DeviceVector) else DeviceVector.from_bytes(points)
        self.k = self.points.n
        h = _vp()
        _check(lib().sc_polytree_build_dev(self.points.ptr, self.k, ctypes.byref(h), None))
        self._h = h

    def zerofier(self):
        out = DeviceVector(self.k + 1)
        _check(lib().sc_polytree_zerofier_dev(self._h, out.ptr, None))
        return out

    def evaluate(self, coeffs):
        """coeffs: DeviceVector of polynomial coefficients (any length) -> DeviceVector of the k values"""
        out = DeviceVector(self.k)
        _check(lib().sc_polytree_evaluate_dev(self._h, coeffs.ptr, coeffs.n, self.points.ptr, out.ptr, None))
        return out

    def interpolate(self, values):
        """values: DeviceVector of k values -> DeviceVector of the k coefficients of the interpolant (degree < k)"""
        assert values.n == self.k
        out = DeviceVector(self.k)
        _check(lib().sc_polytree_interpolate_dev(self._h, values.ptr, out.ptr, None))
        return out

    def evaluate_columns(self, coeff_matrix, m, cols, ld_in=None):
        """coeff_matrix: DeviceVector [cols][m], column c's m coefficients at element c * m (c * ld_in where given) -> DeviceVector
        [cols][k] of the columns' values; every step of `evaluate` issued once per set of columns (sc_polytree_evaluate_columns_dev)"""
        ld_in = m if ld_in is None else ld_in
        assert cols == 0 or coeff_matrix.n >= (cols - 1) * ld_in + m
        out = DeviceVector(max(cols * self.k, 1))
        _check(lib().sc_polytree_evaluate_columns_dev(self._h, coeff_matrix.ptr, m, ld_in, cols, self.points.ptr, out.ptr, self.k, None))
        return out

    def interpolate_columns(self, values_matrix, cols):
        """values_matrix: DeviceVector [cols][k], column c's values at element c * k -> DeviceVector [cols][k] of the columns'
        coefficients; every step of `interpolate` issued once per set of columns (sc_polytree_interpolate_columns_dev)"""
        assert values_matrix.n >= cols * self.k
        out = DeviceVector(max(cols * self.k, 1))
        _check(lib().sc_polytree_interpolate_columns_dev(self._h, values_matrix.ptr, self.k, cols, out.ptr, self.k, None))
        return out

    def interpolate_lagrange(self, values):
        """values: DeviceVector of k values -> DeviceVector of the k coefficients Polynomial.interpolate_domain gives for ANY points:
        a repeated point drops its terms (inverse(0) = 0, code/algebra.py:87-89) where `interpolate` raises; the same coefficients
        for distinct points"""
        assert values.n == self.k
        return self.interpolate_lagrange_columns(values, 1)

    def interpolate_lagrange_columns(self, values_matrix, cols):
        """`interpolate_columns` with those weights (sc_polytree_interpolate_lagrange_columns_dev)"""
        assert values_matrix.n >= cols * self.k
        out = DeviceVector(max(cols * self.k, 1))
        _check(lib().sc_polytree_interpolate_lagrange_columns_dev(self._h, values_matrix.ptr, self.k, cols, out.ptr, self.k, None))
        return out

    def free(self):
        if self._h is not None and _lib is not None:
            _lib.sc_polytree_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class GeoDomain:
    """Owner of an sc_geodomain_t: the tables of a domain that is a geometric progression first * ratio^i, i < n (the trace
    domain {omicron^i} of code/fast_stark.py:84-90).  Same three operations as PolyTree, same results (zerofier, values and
    interpolant are unique), a handful of transforms instead of a tree.  The operations are enqueued on the library stream."""

    def __init__(self, first, ratio, n):
        """first, ratio: int residues; n >= 2 distinct points -- StarkCoreError(unsupported) otherwise (see `create`)"""
        self.first, self.ratio, self.k = int(first), int(ratio), int(n)
        h = _vp()
        _check(lib().sc_geodomain_create(fe_bytes(first), fe_bytes(ratio), self.k, ctypes.byref(h), None))
        self._h = h

    @classmethod
    def create(cls, first, ratio, n):
        """the domain, or None where the progression path does not apply (fewer than two points, repeated points)"""
        dom = cls.__new__(cls)
        dom.first, dom.ratio, dom.k, dom._h = int(first), int(ratio), int(n), None
        h = _vp()
        rc = lib().sc_geodomain_create(fe_bytes(first), fe_bytes(ratio), dom.k, ctypes.byref(h), None)
        if rc == SC_ERR_UNSUPPORTED:
            return None
        _check(rc)
        dom._h = h
        return dom

    @classmethod
    def detect(cls, points):
        """points: DeviceVector.  The GeoDomain of these points if they form a progression of distinct points, else None."""
        if points.n < 2:
            return None
        first, ratio, flag = (ctypes.c_uint64 * 2)(), (ctypes.c_uint64 * 2)(), _int(0)
        _check(lib().sc_geodomain_detect_dev(points.ptr, points.n, first, ratio, ctypes.byref(flag), None))
        if not flag.value:
            return None
        return cls.create(first[0] | (first[1] << 64), ratio[0] | (ratio[1] << 64), points.n)

    def zerofier(self):
        out = DeviceVector(self.k + 1)
        _check(lib().sc_geodomain_zerofier_dev(self._h, out.ptr, None))
        return out

    def evaluate(self, coeffs):
        out = DeviceVector(self.k)
        _check(lib().sc_geodomain_evaluate_dev(self._h, coeffs.ptr, coeffs.n, out.ptr, None))
        return out

    def interpolate(self, values):
        assert values.n == self.k
        out = DeviceVector(self.k)
        _check(lib().sc_geodomain_interpolate_dev(self._h, values.ptr, out.ptr, None))
        return out

    def evaluate_columns(self, coeff_matrix, m, cols, ld_in=None):
        """coeff_matrix: DeviceVector [cols][m], column c's m coefficients at element c * m (c * ld_in where given) -> DeviceVector
        [cols][k] of the columns' values; every step of `evaluate` issued once for all columns (sc_geodomain_evaluate_columns_dev)"""
        ld_in = m if ld_in is None else ld_in
        assert cols == 0 or coeff_matrix.n >= (cols - 1) * ld_in + m
        out = DeviceVector(max(cols * self.k, 1))
        _check(lib().sc_geodomain_evaluate_columns_dev(self._h, coeff_matrix.ptr, m, ld_in, cols, out.ptr, self.k, None))
        return out

    def interpolate_columns(self, values_matrix, cols):
        """values_matrix: DeviceVector [cols][k], column c's values at element c * k -> DeviceVector [cols][k] of the columns'
        coefficients; every step of `interpolate` issued once for all columns (sc_geodomain_interpolate_columns_dev)"""
        assert values_matrix.n >= cols * self.k
        out = DeviceVector(max(cols * self.k, 1))
        _check(lib().sc_geodomain_interpolate_columns_dev(self._h, values_matrix.ptr, self.k, cols, out.ptr, self.k, None))
        return out

    # the points of a progression are distinct, so Polynomial.interpolate_domain's interpolant is the interpolant: the names
    # PolyTree has for it, so that what domain_tables returns is interchangeable
    interpolate_lagrange = interpolate
    interpolate_lagrange_columns = interpolate_columns

    def free(self):
        if self._h is not None and _lib is not None:
            _lib.sc_geodomain_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def domain_tables(points):
    """the device structure that serves fast_zerofier / fast_evaluate / fast_interpolate over `points` (DeviceVector or packed
    bytes): the progression tables where the points are a geometric progression of distinct points, the subproduct tree otherwise"""
    points = points if isinstance(points, DeviceVector) else DeviceVector.from_bytes(points)
    return GeoDomain.detect(points) or PolyTree(points)


_struct_cache = {}


def _digest_struct(count, skipped=0):
    import struct
    st = _struct_cache.get((count, skipped))
    if st is None:
        st = _struct_cache[(count, skipped)] = struct.Struct("64s" * count + ("%dx" % (64 * skipped) if skipped else ""))
    return st


def _path_lists(view, offset, depth, k, keep=None):
    """k authentication paths of `depth` 64-byte digests each, packed back to back in `view` from byte `offset`, as the
    reference's lists of fresh bytes objects (merkle.py:16-27).  One C-level pass per tree: the ~25 000 digest objects of a
    2^22 Fri.prove are the largest host cost of its query phase.  keep < depth: only the first `keep` digests of every path
    become objects (the part of a path below a sharded commitment's sub-roots)."""
    keep = depth if keep is None else min(keep, depth)
    if keep == 0:
        return [[] for _ in range(k)]
    return list(map(list, _digest_struct(keep, depth - keep).iter_unpack(view[offset:offset + 64 * k * depth])))


class MerkleTree:
    """Owner of an sc_merkle_t: all levels resident in HBM, so `open` is a gather (code/merkle.py:16-27)."""

    def __init__(self, handle, root, n):
        self._h = handle
        self._root = root        # None: built asynchronously, fetched (and waited for) on first use
        self.n = n
        self.depth = n.bit_length() - 1

    @property
    def root(self):
        if self._root is None:
            out = ctypes.create_string_buffer(64)
            _check(lib().sc_merkle_root(self._h, out))
            self._root = out.raw
        return self._root

    @classmethod
    def from_device(cls, vec):
        root = ctypes.create_string_buffer(64)
        h = _vp()
        _check(lib().sc_merkle_build_dev(vec.ptr, vec.n, root, ctypes.byref(h), None))
        return cls(h, root.raw, vec.n)

    @classmethod
    def from_device_async(cls, vec):
        """the build is enqueued, not waited for: `.root` waits (the caller prepares its next step meanwhile)"""
        h = _vp()
        _check(lib().sc_merkle_build_async_dev(vec.ptr, vec.n, ctypes.byref(h), None))
        return cls(h, None, vec.n)

    @classmethod
    def from_bytes(cls, data):
        n = len(data) // 16
        root = ctypes.create_string_buffer(64)
        h = _vp()
        _check(lib().sc_merkle_build(bytes(data), n, root, ctypes.byref(h)))
        return cls(h, root.raw, n)

    @classmethod
    def from_device_ptr(cls, ptr, n, stream=None):
        """tree over n field elements at a raw device pointer (e.g. a torch tensor's storage); built on `stream` (a
        ctypes.c_void_p hipStream_t; None = the library's), which is synchronized before the root is returned"""
        root = ctypes.create_string_buffer(64)
        h = _vp()
        _check(lib().sc_merkle_build_dev(ptr, n, root, ctypes.byref(h), stream))
        return cls(h, root.raw, n)

    @classmethod
    def from_device_ptr_async(cls, ptr, n, stream=None):
        """as from_device_ptr, but only enqueued on `stream`: `.root` waits (a caller that needs a level of the tree, not its
        root, never waits at all -- copy_level on the same stream is ordered behind the build)"""
        h = _vp()
        _check(lib().sc_merkle_build_async_dev(ptr, n, ctypes.byref(h), stream))
        return cls(h, None, n)

    @classmethod
    def from_device_ptr_noroot(cls, ptr, n, stream=None):
        """enqueue-only build of a tree whose root is not expected to be read (a rank's local subtree of a sharded commit): no
        pinned root slot, no publish kernel.  `.root` still works, at the price of a device-wide wait."""
        h = _vp()
        _check(lib().sc_merkle_build_noroot_dev(ptr, n, ctypes.byref(h), stream))
        return cls(h, None, n)

    @classmethod
    def from_folded_slab(cls, src_ptr, rows, cols, R, col_base, alpha, offset, omega, dst_ptr, stream=None):
        """the fold of fri.py:85 on a rank's column slab [rows][cols] (sc_fri_fold_slab_dev) AND the enqueue-only local subtree
        over the folded slab, in one library call: the tree's leaf stage computes the fold (alpha, offset, omega: packed bytes)"""
        h = _vp()
        _check(lib().sc_fri_fold_slab_build_dev(src_ptr, rows, cols, R, col_base, alpha, offset, omega, dst_ptr, ctypes.byref(h), stream))
        return cls(h, None, (rows // 2) * cols)

    @classmethod
    def from_digests_ptr(cls, ptr, count, stream=None):
        """tree whose level 0 is `count` given 64-byte digests at a raw device pointer; only enqueued: `.root` waits (polling the
        pinned slot the root is published to)"""
        h = _vp()
        _check(lib().sc_merkle_from_digests_dev(ptr, count, None, ctypes.byref(h), stream))
        return cls(h, None, count)

    def copy_level(self, level, dst_ptr, stream=None):
        """copy the (n >> level) digests of one level into caller-owned device memory"""
        _check(lib().sc_merkle_level_copy_dev(self._h, level, dst_ptr, stream))

    def open_batch(self, indices):
        k = len(indices)
        for i in indices:
            assert 0 <= i < self.n, "cannot open invalid index"
        if k == 0:
            return []
        idx = (ctypes.c_uint64 * k)(*[int(i) for i in indices])
        out = ctypes.create_string_buffer(64 * self.depth * k)
        _check(lib().sc_merkle_open_batch(self._h, idx, k, out))
        # one C-level pass creates all the 64-byte digest objects (they end up, one by one, in the transcript)
        return _path_lists(memoryview(out), 0, self.depth, k)

    def open(self, index):
        return self.open_batch([index])[0]

    def free(self):
        if self._h is not None and _lib is not None:
            _lib.sc_merkle_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


ROWS_MAX_COLUMNS = 256             # SC_MERKLE_ROWS_MAX_COLUMNS of include/starkcore.h


class RowTree(MerkleTree):
    """ONE Merkle tree over the rows of a matrix of codewords (csrc/merkle_rows.cuh): leaf i is the personalised hash
    of every column's value at index i, so a position opens with one path whatever the width.  `columns`: w >= 1 DeviceCodewords,
    DeviceVectors or host sequences (of FieldElements or ints; uploaded) of one power-of-two length.  The tree keeps its columns alive;
    `root`, `open_batch`, `copy_level` and `free` are MerkleTree's."""

    def __init__(self, handle, root, n, vectors):
        super().__init__(handle, root, n)
        self.vectors = vectors
        self.width = len(vectors)
        self._table = (_vp * self.width)(*[v.ptr for v in vectors])

    @staticmethod
    def _vectors(columns):
        vectors = []
        for column in columns:
            if isinstance(column, DeviceCodeword):
                vectors.append(column.vec)
            elif isinstance(column, DeviceVector):
                vectors.append(column)
            else:
                vectors.append(DeviceVector.from_ints([int(getattr(x, "value", x)) for x in column]))
        assert 1 <= len(vectors) <= ROWS_MAX_COLUMNS, "a row tree takes 1 .. %d columns" % ROWS_MAX_COLUMNS
        n = vectors[0].n
        assert all(v.n == n for v in vectors), "columns of one length"
        assert n >= 1 and n & (n - 1) == 0, "length must be power of two"
        return vectors

    @classmethod
    def build(cls, columns):
        vectors = cls._vectors(columns)
        tree = cls(_vp(), None, vectors[0].n, vectors)
        root = ctypes.create_string_buffer(64)
        _check(lib().sc_merkle_rows_build_dev(tree._table, tree.width, tree.n, root, ctypes.byref(tree._h), None))
        tree._root = root.raw
        return tree

    @classmethod
    def start(cls, columns):
        """the build is enqueued, not waited for: `.root` waits (proof_objects.RootLater)"""
        vectors = cls._vectors(columns)
        tree = cls(_vp(), None, vectors[0].n, vectors)
        _check(lib().sc_merkle_rows_build_async_dev(tree._table, tree.width, tree.n, ctypes.byref(tree._h), None))
        return tree

    def query_raw(self, indices):
        """the answers of `query` as the kernel wrote them, into pinned memory of the library's pool: (values, paths) -- uint8 arrays
        of the [k][w] residues (16 bytes each) and of [k][64 * depth] path bytes; the arrays keep the memory alive"""
        k, w, d = len(indices), self.width, self.depth
        for i in indices:
            assert 0 <= i < self.n, "cannot open invalid index"
        self.root                                           # (an asynchronous build has finished once its root is here)
        idx = (ctypes.c_uint64 * max(k, 1))(*[int(i) for i in indices])
        row_bytes = (16 * k * w + 255) & ~255
        out = HostBuffer(row_bytes + max(64 * d * k, 64))
        if k:
            _check(lib().sc_merkle_rows_query_dev(self._h, self._table, w, idx, k, out.ptr, _vp(out.ptr.value + row_bytes)))
        return out.array[:16 * k * w], out.array[row_bytes:row_bytes + 64 * d * k].reshape(k, 64 * d)

    def query(self, indices):
        """(rows, paths) for `indices` in one launch: rows[i] = the w residues (ints) at indices[i], paths[i] its authentication path"""
        k, w = len(indices), self.width
        if k == 0:
            return [], []
        raw, paths = self.query_raw(indices)
        values = unpack(raw.tobytes(), k * w)
        return [values[i * w:(i + 1) * w] for i in range(k)], _path_lists(memoryview(paths).cast("B"), 0, self.depth, k)

    def free(self):
        if self._h is not None and not self._h.value:
            self._h = None                                  # (a build that was refused left no tree)
        super().free()


class CodewordMatrix:
    """K equal-length codewords as ONE device matrix [K][n], row t = member t: what a MerkleForest is built over."""

    def __init__(self, count, n, vec=None):
        self.count, self.n = int(count), int(n)
        self.vec = vec if vec is not None else DeviceVector(self.count * self.n)

    @classmethod
    def from_members(cls, members):
        """members: DeviceCodewords (device copies), packed bytes or sequences of FieldElements (uploads; ONE upload when no member is
        on the device yet), all of one length"""
        members = list(members)
        n = len(members[0]) // 16 if isinstance(members[0], (bytes, bytearray)) else len(members[0])
        rows = []
        for m in members:
            if isinstance(m, DeviceCodeword):
                rows.append(None)
            else:
                rows.append(bytes(m) if isinstance(m, (bytes, bytearray)) else pack(list(map(_value_of, m))))
                assert len(rows[-1]) == 16 * n, "the members of a codeword matrix have one length"
        if all(r is not None for r in rows):
            return cls(len(members), n, DeviceVector.from_bytes(b"".join(rows)))
        matrix = cls(len(members), n)
        for t, (m, r) in enumerate(zip(members, rows)):
            if r is None:
                assert len(m) == n, "the members of a codeword matrix have one length"
                if n:
                    _check(lib().sc_memcpy_dev(_vp(matrix.vec.ptr + 16 * n * t), m.vec.ptr, n, None))
            elif n:
                _check(lib().sc_vec_upload(matrix.vec._h, n * t, r, n))
        return matrix

    def to_bytes(self):
        return self.vec.to_bytes()


class MerkleForest:
    """Owner of an sc_merkle_forest_t: the trees of all rows of a CodewordMatrix, built by one set of launches and resident in HBM.
    `roots` waits for the build (once, for all of them); `open(tree, index)` is a gather."""

    def __init__(self, handle, matrix):
        self._h, self.matrix = handle, matrix
        self.count, self.n = matrix.count, matrix.n
        self.depth = self.n.bit_length() - 1
        self._roots = None

    @classmethod
    def build(cls, matrix):
        h = _vp()
        _check(lib().sc_merkle_forest_build_dev(matrix.vec.ptr, matrix.n, matrix.count, ctypes.byref(h), None))
        return cls(h, matrix)

    @classmethod
    def fold_build(cls, matrix, alphas, offset, omega):
        """one round of Fri.commit for every row (fri.py:85 with the row's own alpha, then the forest of the folded rows), enqueued;
        alphas / offset / omega: int residues"""
        out = CodewordMatrix(matrix.count, matrix.n // 2)
        h = _vp()
        _check(lib().sc_fri_fold_forest_dev(matrix.vec.ptr, matrix.n, matrix.count, pack(alphas), fe_bytes(offset), fe_bytes(omega), out.vec.ptr,
                                            ctypes.byref(h), None))
        return cls(h, out)

    @property
    def roots(self):
        if self._roots is None:
            out = ctypes.create_string_buffer(64 * self.count)
            _check(lib().sc_merkle_forest_roots(self._h, out))
            raw = out.raw
            self._roots = [raw[64 * t:64 * t + 64] for t in range(self.count)]
        return self._roots

    def open(self, tree, index):
        return self.query([(tree, index)])[1][0]

    def query(self, positions):
        """elements (int residues) and authentication paths at positions [(tree, index)]"""
        return query_forests([self], [positions])[0]

    def free(self):
        if self._h is not None and _lib is not None:
            _lib.sc_merkle_forest_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


ROW_FOREST_MAX_SEGMENTS = 8        # SC_ROW_FOREST_MAX_SEGMENTS of include/starkcore.h


class RowSegment(ctypes.Structure):
    """sc_row_segment_t"""
    _fields_ = [("base", _vp), ("per_tree", _u64), ("pitch", _u64)]


class RowForest:
    """Owner of an sc_merkle_forest_t whose leaves are ROWS (csrc/merkle_rows.cuh): `count` row trees of n rows each,
    built by one set of launches.  segments: [(matrix, per_tree) or (matrix, per_tree, pitch)] -- `matrix` a DeviceVector or
    CodewordMatrix of count * per_tree columns, consecutive columns `pitch` (default n) elements apart; tree t's columns are, segment
    after segment, columns t * per_tree ... of that segment.  The forest keeps its matrices alive.  `roots` waits for the build (once)."""

    def __init__(self, handle, matrices, table, n, count):
        self._h, self.matrices, self._table = handle, matrices, table
        self.n, self.count = int(n), int(count)
        self.width = sum(int(segment.per_tree) for segment in table)
        self.depth = self.n.bit_length() - 1
        self._roots = None

    @classmethod
    def build(cls, segments, n, count):
        segments = [tuple(segment) for segment in segments]
        assert 1 <= len(segments) <= ROW_FOREST_MAX_SEGMENTS, "a row forest takes 1 .. %d segments" % ROW_FOREST_MAX_SEGMENTS
        table = (RowSegment * len(segments))()
        matrices = []
        for entry, (matrix, per_tree, *pitch) in zip(table, segments):
            vec = matrix.vec if isinstance(matrix, CodewordMatrix) else matrix
            pitch = n if not pitch or pitch[0] is None else int(pitch[0])
            assert per_tree >= 1 and pitch >= n and vec.n >= (count * per_tree - 1) * pitch + n, "a segment holds count * per_tree columns of n rows"
            entry.base, entry.per_tree, entry.pitch = vec.ptr, int(per_tree), pitch
            matrices.append(matrix)
        forest = cls(_vp(), matrices, table, n, count)
        assert forest.width <= ROWS_MAX_COLUMNS, "a row tree takes 1 .. %d columns" % ROWS_MAX_COLUMNS
        _check(lib().sc_merkle_row_forest_build_dev(table, len(table), n, count, ctypes.byref(forest._h), None))
        return forest

    @property
    def roots(self):
        if self._roots is None:
            out = ctypes.create_string_buffer(64 * self.count)
            _check(lib().sc_merkle_forest_roots(self._h, out))
            raw = out.raw
            self._roots = [raw[64 * t:64 * t + 64] for t in range(self.count)]
        return self._roots

    def query_raw(self, positions):
        """the answers of `query` as the kernel wrote them, into pinned memory of the library's pool: (values, paths) -- uint8 arrays
        of the [k][w] residues (16 bytes each) and of [k][64 * depth] path bytes; the arrays keep the memory alive"""
        k, w, d = len(positions), self.width, self.depth
        for tree, index in positions:
            assert 0 <= tree < self.count and 0 <= index < self.n, "cannot open invalid index"
        trees = (ctypes.c_uint64 * max(k, 1))(*[int(t) for t, _ in positions])
        idx = (ctypes.c_uint64 * max(k, 1))(*[int(i) for _, i in positions])
        row_bytes = (16 * k * w + 255) & ~255
        out = HostBuffer(row_bytes + max(64 * d * k, 64))
        if k:
            _check(lib().sc_merkle_row_forest_query_dev(self._h, self._table, len(self._table), trees, idx, k, out.ptr, _vp(out.ptr.value + row_bytes)))
        return out.array[:16 * k * w], out.array[row_bytes:row_bytes + 64 * d * k].reshape(k, 64 * d)

    def query(self, positions):
        """(rows, paths) for positions [(tree, index)] in one launch: rows[i] = the w residues (ints) of that row, paths[i] its path"""
        k, w = len(positions), self.width
        if k == 0:
            return [], []
        raw, paths = self.query_raw(positions)
        values = unpack(raw.tobytes(), k * w)
        return [values[i * w:(i + 1) * w] for i in range(k)], _path_lists(memoryview(paths).cast("B"), 0, self.depth, k)

    def free(self):
        if self._h is not None and self._h.value and _lib is not None:
            _lib.sc_merkle_forest_free(self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def forest_stats():
    """(forests built, trees in them) so far"""
    out = (ctypes.c_uint64 * 2)()
    _check(lib().sc_merkle_forest_stats(out))
    return out[0], out[1]


def query_forests(forests, requests):
    """openings of several forests in ONE device round trip: requests[p] = [(tree, index)] into forests[p]; returns per pair
    (int residues, paths as lists of fresh 64-byte digests).  The kernel writes into pinned memory of the library's pool."""
    n = len(forests)
    try:
        trees = array.array("Q", [t for req in requests for t, _ in req])
        flat = array.array("Q", [i for req in requests for _, i in req])
    except OverflowError:
        raise AssertionError("cannot open invalid index")
    total = len(flat)
    if total == 0:
        return [([], []) for _ in forests]
    depths = [f.depth for f in forests]
    el_bytes = (16 * total + 255) & ~255
    path_bytes = sum(64 * d * len(req) for d, req in zip(depths, requests))
    answers = HostBuffer(el_bytes + max(path_bytes, 64))
    _check(lib().sc_merkle_forest_query_dev(n, (_vp * n)(*[f._h for f in forests]), (_vp * n)(*[f.matrix.vec.ptr for f in forests]),
                                            (ctypes.c_uint64 * total).from_buffer(trees), (ctypes.c_uint64 * total).from_buffer(flat),
                                            (ctypes.c_uint64 * n)(*[len(req) for req in requests]), answers.ptr, _vp(answers.ptr.value + el_bytes)))
    data = answers.array
    values = unpack(data[:16 * total].tobytes(), total)
    view = memoryview(data[el_bytes:].tobytes())
    out, vo, po = [], 0, 0
    for req, d in zip(requests, depths):
        k = len(req)
        out.append((values[vo:vo + k], _path_lists(view, po, d, k)))
        vo += k
        po += 64 * k * d
    return out


import operator as _operator

_value_of = _operator.attrgetter("value")
_FieldElement = None


def _field_element():
    """algebra.FieldElement, imported on first use (algebra does not depend on this module, but importing it at load time would
    make every C-ABI-only user pay for it)"""
    global _FieldElement
    if _FieldElement is None:
        from algebra import FieldElement
        _FieldElement = FieldElement
    return _FieldElement


class DeviceCodeword(Sequence):
    """A list-like view of a device-resident codeword.

    Behaves like the `list[FieldElement]` the reference passes around (len, indexing, iteration,
    equality with lists) but keeps the data in HBM; `Fri` and `Merkle` recognise it and stay on the
    device.  Elements are materialised as FieldElement only when asked for.
    """

    def __init__(self, vec, field, elements=None):
        self.vec = vec
        self.field = field
        self._tree = None
        # index -> FieldElement.  Identity matters: the Fiat-Shamir transcript is pickle.dumps(objects)
        # (code/ip.py:18-25) and pickle memoises by object identity; the reference pushes the SAME
        # FieldElement object when a codeword entry appears twice (last codeword + query triple, or the `c`
        # of one round and the `a`/`b` of the next: code/fri.py:91,104-105), so entries are created once.
        self._elems = {}
        self._full = None
        if elements is not None:
            self._full = elements
            self._elems = None

    # -- construction helpers
    @classmethod
    def from_list(cls, values, field):
        values = list(values)
        return cls(DeviceVector.from_ints(list(map(_value_of, values))), field, elements=values)

    def __len__(self):
        return self.vec.n

    def _fe(self, v):
        return _field_element()(v, self.field)

    def tolist(self):
        if self._full is None:
            known = self._elems
            ints = unpack(self.vec.to_bytes(), self.vec.n)
            self._full = [known[i] if i in known else self._fe(v) for i, v in enumerate(ints)]
            holder = getattr(self, "_proof_entries", None)
            if holder is not None:                          # a proof stream describes entries of this codeword: it shares the
                known.update(enumerate(self._full))         # cache that is retired here and must know every object
            self._elems = None
        return self._full

    def __getitem__(self, i):
        if isinstance(i, slice):
            return self.tolist()[i]
        n = self.vec.n
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError("codeword index out of range")
        return self.gather([i])[0]

    def gather(self, indices):
        """Entries at `indices` (one D2H gather for the ones not materialised yet)."""
        if self._full is not None:
            return [self._full[i] for i in indices]
        known = self._elems
        missing = [i for i in dict.fromkeys(indices) if i not in known]
        if missing:
            for i, v in zip(missing, self.vec.gather(missing)):
                known[i] = self._fe(v)
        return [known[i] for i in indices]

    def __iter__(self):
        return iter(self.tolist())

    def __eq__(self, other):
        if isinstance(other, DeviceCodeword):
            return self.vec.to_bytes() == other.vec.to_bytes()
        return self.tolist() == list(other)

    __hash__ = None

    def tree(self):
        if self._tree is None:
            self._tree = MerkleTree.from_device(self.vec)
        return self._tree

    def start_tree(self):
        """enqueue the build of the tree and return at once (`tree().root` waits for it)"""
        if self._tree is None:
            self._tree = MerkleTree.from_device_async(self.vec)
        return self._tree

    def fold_commit(self, alpha, offset, omega, out_vec):
        """One round of Fri.commit in one library call (fri.py:85 then the tree of the folded codeword, both only enqueued):
        the folded DeviceCodeword, whose tree().root waits for the device."""
        h = _vp()
        _check(lib().sc_fri_fold_commit_dev(self.vec.ptr, self.vec.n, fe_bytes(alpha.value), fe_bytes(offset.value), fe_bytes(omega.value),
                                            out_vec.ptr, ctypes.byref(h), None))
        folded = DeviceCodeword(out_vec, self.field)
        folded._tree = MerkleTree(h, None, out_vec.n)
        return folded

    # -- pair leaves (Fri(pair_leaves=True)): the codeword under the row tree of its two halves
    def _halves(self):
        """the two halves as vectors over this codeword's memory: two pointers into the one vector, no copy"""
        n = self.vec.n
        assert n >= 2 and n & (n - 1) == 0, "a pair tree needs a power-of-two length of at least 2"
        base = int(self.vec.ptr)
        return [DeviceVector.wrap(base, n // 2, self.vec), DeviceVector.wrap(base + 8 * n, n // 2, self.vec)]

    def pair_tree(self):
        if getattr(self, "_pair_tree", None) is None:
            self._pair_tree = RowTree.build(self._halves())
        return self._pair_tree

    def start_pair_tree(self):
        """enqueue the build of the pair tree and return at once (`pair_tree().root` waits for it)"""
        if getattr(self, "_pair_tree", None) is None:
            self._pair_tree = RowTree.start(self._halves())
        return self._pair_tree

    def fold_pairs_commit(self, alpha, offset, omega, out_vec):
        """fold_commit with pair leaves (sc_fri_fold_pairs_commit_dev): the folded DeviceCodeword, whose pair_tree().root waits for
        the device"""
        h = _vp()
        _check(lib().sc_fri_fold_pairs_commit_dev(self.vec.ptr, self.vec.n, fe_bytes(alpha.value), fe_bytes(offset.value), fe_bytes(omega.value),
                                                  out_vec.ptr, ctypes.byref(h), None))
        folded = DeviceCodeword(out_vec, self.field)
        folded._pair_tree = MerkleTree(h, None, out_vec.n // 2)
        return folded

    def query(self, indices):
        """One device round trip: the entries at `indices` (identity-preserving, like gather) and one freshly created
        authentication path per requested index (paths are new objects every time, as in the reference, which
        recomputes them per Merkle.open call)."""
        tree = self.tree()
        k = len(indices)
        if k == 0:
            return [], []
        idx = (ctypes.c_uint64 * k)(*[int(i) for i in indices])
        d = tree.depth
        elems = ctypes.create_string_buffer(16 * k)
        paths = ctypes.create_string_buffer(64 * d * k if d else 64)
        _check(lib().sc_merkle_query_dev(tree._h, self.vec.ptr, idx, k, elems, paths))
        return self._entries(indices, unpack(elems.raw, k)), _path_lists(memoryview(paths), 0, d, k)

    def _entries(self, indices, values):
        """FieldElement objects for freshly fetched residues, created once per index (see __init__)"""
        if self._full is not None:
            return [self._full[i] for i in indices]
        known, fe, field, new = self._elems, _field_element(), self.field, object.__new__
        for i, v in zip(indices, values):
            if i not in known:
                # FieldElement(v, field) without the call into __init__ (algebra.py:16-18 sets exactly these two attributes):
                # half the cost per object, and a query phase creates over a thousand of them
                e = new(fe)
                e.value = v
                e.field = field
                known[i] = e
        return [known[i] for i in indices]
