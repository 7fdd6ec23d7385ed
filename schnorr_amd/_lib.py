"""ctypes binding of libdsv.so (include/dsv.h).  There is NO CPU fallback: if the library is
missing or a call fails, an exception is raised."""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DSV_LIB_PATH") or os.path.join(HERE, "libdsv.so")  # override: A/B builds

# every extern "C" symbol include/dsv.h declares
SYMBOLS = [
    "dsv_init", "dsv_shutdown", "dsv_version", "dsv_last_error", "dsv_device_count",
    "dsv_verify_single", "dsv_verify_double", "dsv_verify_vargen", "dsv_verify_single_ext",
    "dsv_workspace_bytes", "dsv_verify_single_dev", "dsv_verify_double_dev",
    "dsv_verify_vargen_dev", "dsv_verify_core_dev", "dsv_challenge_single", "dsv_challenge_double",
    "dsv_challenge_single_dev", "dsv_challenge_double_dev", "dsv_sign_single", "dsv_sign_double",
    "dsv_sign_vargen", "dsv_public_keys", "dsv_sign_single_dev", "dsv_sign_double_dev",
    "dsv_public_keys_dev", "dsv_compress_points", "dsv_decompress_points", "dsv_decompress_points_dev",
    "dsv_verify_single_wire", "dsv_verify_double_wire", "dsv_verify_vargen_wire",
    "dsv_stdrng_sign_inputs", "dsv_stdrng_sign_inputs_dev",
    "dsv_debug_table_entry", "dsv_fixed_window_bits", "dsv_debug_fq_mul",
    # r02: several devices per process, fused double kernel, mixed batches, var-generator inputs
    "dsv_shutdown_device", "dsv_set_device", "dsv_get_device", "dsv_initialized_devices",
    "dsv_verify_single_multi", "dsv_verify_double_multi", "dsv_verify_vargen_multi",
    "dsv_verify_core_double_dev", "dsv_mixed_workspace_bytes", "dsv_verify_mixed_dev",
    "dsv_split_scratch_bytes", "dsv_split_kinds_dev", "dsv_gather_rows_dev",
    "dsv_scatter_verdicts_dev", "dsv_public_keys_vargen_dev", "dsv_sign_vargen_dev",
    "dsv_stdrng_vargen_inputs_dev",
    # r03: projective inputs for every scheme (host / multi-device / device pointers), wire records
    # in device memory, one-call initialisation
    "dsv_init_visible", "dsv_to_hash_inputs", "dsv_debug_lattice3", "dsv_debug_half_scalars",
    "dsv_verify_double_ext", "dsv_verify_vargen_ext",
    "dsv_verify_single_ext_multi", "dsv_verify_double_ext_multi", "dsv_verify_vargen_ext_multi",
    "dsv_ext_workspace_bytes", "dsv_verify_single_ext_dev", "dsv_verify_double_ext_dev",
    "dsv_verify_vargen_ext_dev",
    "dsv_wire_workspace_bytes", "dsv_verify_single_wire_dev", "dsv_verify_double_wire_dev",
    "dsv_verify_vargen_wire_dev",
    # r04: the reference's in-memory representation (Montgomery limbs), dense arrays / strided
    # columns of typed objects / device pointers
    "dsv_verify_single_mont", "dsv_verify_double_mont", "dsv_verify_vargen_mont",
    "dsv_verify_single_mont_multi", "dsv_verify_double_mont_multi", "dsv_verify_vargen_mont_multi",
    "dsv_verify_single_mont_cols", "dsv_verify_double_mont_cols", "dsv_verify_vargen_mont_cols",
    "dsv_mont_workspace_bytes", "dsv_verify_single_mont_dev", "dsv_verify_double_mont_dev",
    "dsv_verify_vargen_mont_dev", "dsv_set_host_threads",
    # r05: asynchronous form of the column entry points (two batches in flight per device)
    "dsv_verify_single_mont_cols_submit", "dsv_verify_double_mont_cols_submit",
    "dsv_verify_vargen_mont_cols_submit", "dsv_job_wait", "dsv_job_done", "dsv_max_in_flight",
    # r05: random-linear-combination fast accept in front of the per-signature kernels
    "dsv_rlc_workspace_bytes", "dsv_verify_single_rlc_dev", "dsv_verify_double_rlc_dev",
    "dsv_verify_vargen_rlc_dev", "dsv_rlc_plan_info", "dsv_debug_rlc_history", "dsv_debug_rlc_history_long", "dsv_debug_rlc_subgroups", "dsv_device_numa", "dsv_debug_numa_lookup",
    "dsv_verify_single_mont_cols_rlc", "dsv_verify_double_mont_cols_rlc", "dsv_verify_vargen_mont_cols_rlc",
    "dsv_wire_rlc_workspace_bytes", "dsv_verify_single_wire_rlc_dev", "dsv_verify_double_wire_rlc_dev",
    "dsv_verify_vargen_wire_rlc_dev",
    "dsv_verify_single_wire_rlc", "dsv_verify_double_wire_rlc", "dsv_verify_vargen_wire_rlc",
    "dsv_mixed_rlc_workspace_bytes", "dsv_verify_mixed_rlc_dev",
    # registered key sets: verify by key index with per-key fixed-base tables
    "dsv_keyset_bytes", "dsv_keyset_create", "dsv_keyset_create_wire", "dsv_keyset_destroy", "dsv_keyset_info",
    "dsv_keyset_key_ok", "dsv_keyed_workspace_bytes", "dsv_verify_single_keyed_dev", "dsv_verify_double_keyed_dev",
    "dsv_verify_vargen_keyed_dev", "dsv_verify_single_keyed", "dsv_verify_double_keyed", "dsv_verify_vargen_keyed",
    "dsv_debug_keyset_entry",
    # keyed fast accept: the batch aggregate over a registered key set
    "dsv_keyed_rlc_workspace_bytes", "dsv_keyed_rlc_plan_info", "dsv_debug_keyed_rlc_history",
    "dsv_verify_single_keyed_rlc_dev", "dsv_verify_double_keyed_rlc_dev", "dsv_verify_vargen_keyed_rlc_dev",
    # keyed wire form: serialized signatures against a registered key set
    "dsv_keyed_wire_workspace_bytes", "dsv_verify_single_keyed_wire_dev", "dsv_verify_double_keyed_wire_dev",
    "dsv_verify_vargen_keyed_wire_dev", "dsv_verify_single_keyed_wire", "dsv_verify_double_keyed_wire",
    "dsv_verify_vargen_keyed_wire",
    # keyed typed-object form: the reference's in-memory objects against a registered key set
    "dsv_keyset_create_mont_cols", "dsv_keyed_mont_workspace_bytes", "dsv_verify_keyed_mont_dev",
    "dsv_verify_keyed_mont_cols", "dsv_verify_keyed_mont_cols_submit",
    # key sets by key value: the index over a set's keys, lookup, closed-set verify
    "dsv_keyset_index_bytes", "dsv_keyset_lookup_dev", "dsv_keyset_lookup", "dsv_keyed_lookup_workspace_bytes",
    "dsv_verify_keyed_lookup_dev", "dsv_verify_keyed_lookup", "dsv_debug_keyset_home_slot",
    "dsv_debug_keyset_index_stats",
    # key sets as a key cache: open-set verify by key value (misses take the unkeyed equation in the same call)
    "dsv_keyed_open_workspace_bytes", "dsv_verify_keyed_open_dev", "dsv_verify_keyed_open",
    # ... and the var-generator scheme's open-set form (key columns PK, Gen)
    "dsv_verify_vargen_keyed_open_dev", "dsv_verify_vargen_keyed_open",
    # key sets that grow: reserved capacity, keys appended to a live set
    "dsv_keyset_create_reserved", "dsv_keyset_append", "dsv_keyset_append_wire", "dsv_keyset_append_mont_cols",
    "dsv_keyset_capacity", "dsv_keyset_key_ok_n",
    # the key cache for serialized records: the wire index, open-set verify by compressed key
    "dsv_keyset_wire_index_bytes", "dsv_keyset_lookup_wire_dev", "dsv_keyset_lookup_wire",
    "dsv_debug_keyset_wire_home_slot", "dsv_keyed_open_wire_workspace_bytes",
    "dsv_verify_single_keyed_open_wire_dev", "dsv_verify_double_keyed_open_wire_dev",
    "dsv_verify_vargen_keyed_open_wire_dev", "dsv_verify_single_keyed_open_wire",
    "dsv_verify_double_keyed_open_wire", "dsv_verify_vargen_keyed_open_wire",
    # keys replaced in place: the key cache's eviction
    "dsv_keyset_replace", "dsv_keyset_replace_wire", "dsv_debug_keyset_slots", "dsv_debug_keyset_replace_exclusive_ns",
    # the key cache for typed objects: open-set verify of verify_batch's arguments
    "dsv_keyed_open_mont_workspace_bytes", "dsv_verify_keyed_open_mont_dev", "dsv_verify_keyed_open_mont_cols",
    "dsv_verify_keyed_open_mont_cols_submit",
]
_SIZE_T_FUNCS = ("dsv_workspace_bytes", "dsv_mixed_workspace_bytes", "dsv_split_scratch_bytes",
                 "dsv_ext_workspace_bytes", "dsv_wire_workspace_bytes", "dsv_mont_workspace_bytes",
                 "dsv_rlc_workspace_bytes", "dsv_wire_rlc_workspace_bytes", "dsv_mixed_rlc_workspace_bytes",
                 "dsv_keyset_bytes", "dsv_keyed_workspace_bytes", "dsv_keyed_rlc_workspace_bytes",
                 "dsv_keyed_wire_workspace_bytes", "dsv_keyed_mont_workspace_bytes",
                 "dsv_keyset_index_bytes", "dsv_keyed_lookup_workspace_bytes", "dsv_keyed_open_workspace_bytes",
                 "dsv_keyset_wire_index_bytes", "dsv_keyed_open_wire_workspace_bytes",
                 "dsv_keyed_open_mont_workspace_bytes")


class Column(ctypes.Structure):
    """dsv_column: one field of n typed objects, item i at base + i * stride"""
    _fields_ = [("base", ctypes.c_void_p), ("stride", ctypes.c_size_t)]


class DsvError(RuntimeError):
    pass


_lib = None


def load():
    """Load libdsv.so (building it first if hipcc is available and it is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        from . import build as _build  # raises if hipcc is absent

        _build.build()
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 and libdsv.so is linked
    # against the system one.  If libdsv (and with it the system runtime) is loaded first, a later
    # `import torch` + CUDA init in the same process fails with "No HIP GPUs are available"; in the
    # other order the dynamic loader resolves libdsv's dependency to the copy torch already
    # mapped.  The device-tensor entry points of this package need torch anyway, so load it first
    # when it is installed.  (Pure C / Rust callers never see this: they have one runtime.)
    try:
        import torch  # noqa: F401
    except ImportError:  # pragma: no cover
        pass
    try:
        L = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise DsvError("cannot load the HIP engine %s: %s" % (LIB_PATH, e))
    L.dsv_version.restype = ctypes.c_char_p
    L.dsv_last_error.restype = ctypes.c_char_p
    for name in _SIZE_T_FUNCS:
        getattr(L, name).restype = ctypes.c_size_t
        getattr(L, name).argtypes = [ctypes.c_size_t] + ([ctypes.c_int] if name in ("dsv_rlc_workspace_bytes", "dsv_wire_rlc_workspace_bytes") else [])
    L.dsv_keyset_bytes.argtypes = [ctypes.c_int, ctypes.c_size_t]
    L.dsv_keyed_wire_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_size_t]
    L.dsv_keyed_mont_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_size_t]
    L.dsv_keyed_rlc_workspace_bytes.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int]
    L.dsv_keyset_index_bytes.argtypes = [ctypes.c_int, ctypes.c_size_t]
    L.dsv_keyset_wire_index_bytes.argtypes = [ctypes.c_int, ctypes.c_size_t]
    L.dsv_keyed_open_wire_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_size_t]
    L.dsv_debug_keyset_wire_home_slot.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    L.dsv_debug_keyset_home_slot.restype = ctypes.c_uint64
    L.dsv_debug_keyset_home_slot.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.dsv_keyset_replace.argtypes = [vp, vp, vp, vp, sz]
    L.dsv_keyset_replace_wire.argtypes = [vp, vp, vp, sz]
    L.dsv_debug_keyset_slots.argtypes = [vp, ctypes.c_int, vp, sz, vp]
    L.dsv_debug_keyset_replace_exclusive_ns.restype = ctypes.c_uint64
    # (ks, u, R, PK, Gen, m, n, ok, workspace, workspace_bytes, stream, misses) / (ks, u, R, PK, Gen, m, n, ok, misses)
    L.dsv_verify_vargen_keyed_open_dev.argtypes = [vp] * 6 + [sz, vp, vp, sz, vp, vp]
    L.dsv_verify_vargen_keyed_open.argtypes = [vp] * 6 + [sz, vp, vp]
    for scheme in ("single", "double", "vargen"):
        # (ks, sig, pk, m, n, ok, workspace, workspace_bytes, stream, misses) / (ks, sig, pk, m, n, ok, misses)
        getattr(L, "dsv_verify_%s_keyed_open_wire_dev" % scheme).argtypes = [vp] * 4 + [sz, vp, vp, sz, vp, vp]
        getattr(L, "dsv_verify_%s_keyed_open_wire" % scheme).argtypes = [vp] * 4 + [sz, vp, vp]
    L.dsv_keyset_lookup_wire_dev.argtypes = [vp, vp, sz, vp, vp, vp]
    L.dsv_keyed_open_mont_workspace_bytes.argtypes = [ctypes.c_int, sz]
    # (ks, u, R, Rp, key_a, key_b, m, n, ok, workspace, workspace_bytes, stream, misses)
    L.dsv_verify_keyed_open_mont_dev.argtypes = [vp] * 7 + [sz, vp, vp, sz, vp, vp]
    L.dsv_verify_keyed_open_mont_cols.argtypes = [vp, vp, sz, vp, vp]         # (ks, cols, n, ok, misses)
    L.dsv_verify_keyed_open_mont_cols_submit.argtypes = [vp, vp, sz, vp, vp]  # (ks, cols, n, ok, job)
    L.dsv_keyset_lookup_wire.argtypes = [vp, vp, sz, vp, vp]
    for name in SYMBOLS:
        fn = getattr(L, name)  # AttributeError if a declared symbol is not exported
        if name not in ("dsv_version", "dsv_last_error", "dsv_debug_keyset_home_slot",
                        "dsv_debug_keyset_replace_exclusive_ns") + _SIZE_T_FUNCS:
            fn.restype = ctypes.c_int
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise DsvError("dsv error %d: %s" % (rc, load().dsv_last_error().decode()))
