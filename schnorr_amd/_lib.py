"""ctypes binding of libdsv.so (include/dsv.h).  There is NO CPU fallback: if the library is
missing or a call fails, an exception is raised."""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DSV_LIB_PATH") or os.path.join(HERE, "libdsv.so")  # override: A/B builds

# ---- the signature table: every extern "C" function include/dsv.h declares, written once -----------------------
# A signature is a string of one-letter codes, the result first and then one per parameter:
#   i int    z size_t    q uint64_t    s const char *    p any other pointer (arrays and dsv_job ** included)
# load() sets restype and argtypes of every symbol from it, so ctypes converts plain Python ints, None and
# byref(...) itself and refuses a missing, surplus or mistyped argument.  A new export needs one entry here
# and nothing else; tests/test_lib_signatures.py compares the table with the header's prototypes.
_CTYPES = {"i": ctypes.c_int, "z": ctypes.c_size_t, "q": ctypes.c_uint64, "s": ctypes.c_char_p,
           "p": ctypes.c_void_p}


def _signatures():
    t = {}

    def add(sig, *names):
        for name in names:
            assert name not in t, name
            t[name] = sig

    # lifecycle, devices, NUMA placement
    add("i", "dsv_init_visible", "dsv_shutdown", "dsv_get_device", "dsv_device_count", "dsv_max_in_flight",
        "dsv_fixed_window_bits")
    add("ii", "dsv_init", "dsv_shutdown_device", "dsv_set_device", "dsv_set_host_threads", "dsv_debug_rlc_subgroups")
    add("s", "dsv_version", "dsv_last_error")
    add("ipi", "dsv_initialized_devices")                       # (out, cap)
    add("iippip", "dsv_device_numa")                            # (device, node, cpus, cap, bdf)
    add("issppi", "dsv_debug_numa_lookup")                      # (sysfs_root, bdf, node, cpus, cap)
    add("ip", "dsv_job_wait", "dsv_job_done", "dsv_keyset_destroy")
    # the verify family of each scheme.  fields: u, the points in the scheme's order, m; keys: the points that are
    # the key, which the keyed forms replace by ONE index column behind a leading key-set handle
    for scheme, fields, keys in (("single", 4, 1), ("double", 6, 2), ("vargen", 5, 2)):
        v = "dsv_verify_" + scheme
        item = "i" + "p" * fields
        for form in ("", "_ext", "_mont"):                      # affine / projective / Montgomery limbs
            add(item + "zp", v + form, v + form + "_multi")     # (..., n, ok)
            add(item + "zppp", v + form + "_dev")               # (..., n, ok, workspace, stream)
        add(item + "zpppip", v + "_rlc_dev")                    # (..., stream, window_bits, accepted)
        add("ipzp", v + "_mont_cols")                           # (cols, n, ok)
        add("ipzpp", v + "_mont_cols_rlc", v + "_mont_cols_submit")  # (cols, n, ok, accepted | job)
        add("ipppzp", v + "_wire")                              # (sig, pk, m, n, ok)
        add("ipppzpp", v + "_wire_rlc")                         # (..., accepted)
        add("ipppzppp", v + "_wire_dev")                        # (sig, pk, m, n, ok, workspace, stream)
        add("ipppzpppip", v + "_wire_rlc_dev")                  # (..., window_bits, accepted)
        keyed = "i" + "p" * (fields - keys + 2)                 # (ks, u, R[, Rp], key_idx, m, ...
        add(keyed + "zp", v + "_keyed")                         # ..., n, ok)
        add(keyed + "zppzp", v + "_keyed_dev")                  # ..., n, ok, workspace, workspace_bytes, stream)
        add(keyed + "zppzpip", v + "_keyed_rlc_dev")            # ..., stream, window_bits, accepted)
        add("ippppzp", v + "_keyed_wire")                       # (ks, sig, key_idx, m, n, ok)
        add("ippppzppzp", v + "_keyed_wire_dev")                # (..., workspace, workspace_bytes, stream)
        add("ippppzpp", v + "_keyed_open_wire")                 # (ks, sig, pk, m, n, ok, misses)
        add("ippppzppzpp", v + "_keyed_open_wire_dev")          # (..., ok, workspace, workspace_bytes, stream, misses)
    # workspace and table sizes (no GPU needed)
    add("zz", "dsv_workspace_bytes", "dsv_ext_workspace_bytes", "dsv_mont_workspace_bytes",
        "dsv_wire_workspace_bytes", "dsv_mixed_workspace_bytes", "dsv_mixed_rlc_workspace_bytes",
        "dsv_split_scratch_bytes", "dsv_keyed_workspace_bytes", "dsv_keyed_lookup_workspace_bytes",
        "dsv_keyed_open_workspace_bytes")                       # (n)
    add("zzi", "dsv_rlc_workspace_bytes", "dsv_wire_rlc_workspace_bytes")  # (n, window_bits)
    add("zzzi", "dsv_keyed_rlc_workspace_bytes")                # (n, k, window_bits)
    add("ziz", "dsv_keyset_bytes", "dsv_keyset_index_bytes", "dsv_keyset_wire_index_bytes",
        "dsv_keyed_wire_workspace_bytes", "dsv_keyed_mont_workspace_bytes", "dsv_keyed_open_wire_workspace_bytes",
        "dsv_keyed_open_mont_workspace_bytes")                  # (scheme, k | n)
    # the batch fast accept's plans and history counters
    add("iiziip", "dsv_rlc_plan_info")                          # (scheme, n, window_bits, groups, out[24])
    add("iizziip", "dsv_keyed_rlc_plan_info")                   # (scheme, n, k, window_bits, groups, out[24])
    add("iii", "dsv_debug_rlc_history", "dsv_debug_rlc_history_long", "dsv_debug_keyed_rlc_history")  # (device, set)
    # second stages alone, mixed batches and their pieces (device pointers)
    add("ipppppiizppp", "dsv_verify_core_dev")   # (u, c, valid, PK, R, which, accumulate, n, ok, workspace, stream)
    add("ipppppppzppp", "dsv_verify_core_double_dev")  # (u, c, valid, PK, R, PKp, Rp, n, ok, workspace, stream)
    add("ipppppppzzppp", "dsv_verify_mixed_dev")  # (kinds, u, R, Rp, PK, PKp, m, n, n_double, ok, workspace, stream)
    add("ipppppppzzpppp", "dsv_verify_mixed_rlc_dev")           # (..., accepted)
    add("ipzpzpzpp", "dsv_split_kinds_dev")  # (kinds, n, idx_single, cap_single, idx_double, cap_double, scratch,
    #                                           stream)
    add("ipzzpzppp", "dsv_gather_rows_dev")  # (src, src_rows, row_bytes, idx, count, count_limit, dst, stream)
    add("ippzppzp", "dsv_scatter_verdicts_dev")                 # (src, idx, count, count_limit, dst, dst_len, stream)
    # challenge hash, signing and key derivation, wire formats, the reference harness's input generator
    add("ippzp", "dsv_challenge_single")                        # (R, m, n, c)
    add("ipppzp", "dsv_challenge_double")                       # (R, Rp, m, n, c)
    add("ippzppp", "dsv_challenge_single_dev")                  # (R, m, n, c, valid, stream)
    add("ipppzppp", "dsv_challenge_double_dev")
    add("ipppzpp", "dsv_sign_single")                           # (sk, m, r, n, u, R)
    add("ipppzppp", "dsv_sign_double", "dsv_sign_single_dev")   # (..., Rp) / (..., stream)
    add("ipppzpppp", "dsv_sign_double_dev")
    add("ippppzpp", "dsv_sign_vargen")                          # (sk, Gen, m, r, n, u, R)
    add("ippppzpppp", "dsv_sign_vargen_dev")                    # (..., workspace, stream)
    add("ipipzp", "dsv_public_keys")                            # (sk, which, gen, n, PK)
    add("ipizpp", "dsv_public_keys_dev")                        # (sk, which, n, PK, stream)
    add("ippzppp", "dsv_public_keys_vargen_dev")                # (sk, Gen, n, PK, workspace, stream)
    add("ipzp", "dsv_compress_points", "dsv_debug_half_scalars")  # (in, n, out)
    add("ipzpp", "dsv_decompress_points", "dsv_to_hash_inputs")  # (in, n, out, ok)
    add("ipzzppip", "dsv_decompress_points_dev")                # (in, in_stride, n, out, ok, accumulate, stream)
    add("iqzzppp", "dsv_stdrng_sign_inputs")                    # (seed, first_item, n, sk, m, r)
    add("iqzzpppp", "dsv_stdrng_sign_inputs_dev")               # (..., stream)
    add("iqzzppppp", "dsv_stdrng_vargen_inputs_dev")            # (seed, first_item, n, sk, g, m, r, stream)
    add("iiiip", "dsv_debug_table_entry")                       # (which, window, digit, out96)
    add("ippzp", "dsv_debug_lattice3", "dsv_debug_fq_mul")      # (a, b, n, out)
    # key sets: constructors, growth, replacement, inspection
    add("iippzp", "dsv_keyset_create")                          # (scheme, pk, pk2, k, out)
    add("iippzzp", "dsv_keyset_create_reserved")                # (scheme, pk, pk2, k, capacity, out)
    add("iipzp", "dsv_keyset_create_wire", "dsv_keyset_create_mont_cols")  # (scheme, records | cols, k, out)
    add("ipppzp", "dsv_keyset_append")                          # (ks, pk, pk2, m, first_index)
    add("ippzp", "dsv_keyset_append_wire", "dsv_keyset_append_mont_cols", "dsv_keyset_key_ok_n")
    add("ippppz", "dsv_keyset_replace")                         # (ks, indices, pk, pk2, m)
    add("ipppz", "dsv_keyset_replace_wire")                     # (ks, indices, records, m)
    add("ippppp", "dsv_keyset_info")                            # (ks, scheme, k, bytes, device)
    add("ipp", "dsv_keyset_key_ok", "dsv_keyset_capacity", "dsv_debug_keyset_index_stats")
    add("ipziiip", "dsv_debug_keyset_entry")                    # (ks, key, point, window, digit, out64)
    add("ipipzp", "dsv_debug_keyset_slots")                     # (ks, form, out, room, slots)
    add("qizpp", "dsv_debug_keyset_home_slot")                  # (scheme, k, key_a, key_b) -> slot
    add("iizpp", "dsv_debug_keyset_wire_home_slot")             # (scheme, capacity, record, slot)
    add("q", "dsv_debug_keyset_replace_exclusive_ns")
    # key sets: typed objects by key index, lookup and verify by key value (closed set, open set = key cache)
    add("ippppppzppzp", "dsv_verify_keyed_mont_dev")  # (ks, u, R, Rp, idx, m, n, ok, ws, ws_bytes, stream)
    add("ippzp", "dsv_verify_keyed_mont_cols")                  # (ks, cols, n, ok)
    add("ippzpp", "dsv_verify_keyed_mont_cols_submit", "dsv_verify_keyed_open_mont_cols",
        "dsv_verify_keyed_open_mont_cols_submit", "dsv_keyset_lookup_wire")  # (..., job | misses)
    add("ipppzpp", "dsv_keyset_lookup")                         # (ks, key_a, key_b, n, idx, misses)
    add("ipppzppp", "dsv_keyset_lookup_dev")                    # (ks, key_a, key_b, n, idx, misses, stream)
    add("ippzppp", "dsv_keyset_lookup_wire_dev")                # (ks, pk, n, idx, misses, stream)
    # (ks, u, R, Rp, key_a, key_b, m, n, ok, misses) / (..., n, ok, workspace, workspace_bytes, stream, misses)
    add("ipppppppzpp", "dsv_verify_keyed_lookup", "dsv_verify_keyed_open")
    add("ipppppppzppzpp", "dsv_verify_keyed_lookup_dev", "dsv_verify_keyed_open_dev",
        "dsv_verify_keyed_open_mont_dev")
    add("ippppppzpp", "dsv_verify_vargen_keyed_open")           # (ks, u, R, PK, Gen, m, n, ok, misses)
    add("ippppppzppzpp", "dsv_verify_vargen_keyed_open_dev")
    # key cache census: per-key hit counts and the distinct missed keys
    add("zz", "dsv_keyset_census_workspace_bytes")              # (n)
    add("ziz", "dsv_keyset_census_mont_workspace_bytes")        # (scheme, n)
    # (ks, key_a, key_b, n, idx, hits, rep, count, totals[, workspace, workspace_bytes, stream])
    add("ipppzppppp", "dsv_keyset_census")
    add("ipppzppppppzp", "dsv_keyset_census_dev", "dsv_keyset_census_mont_dev")
    # (ks, records | cols, n, idx, hits, rep, count, totals[, workspace, workspace_bytes, stream])
    add("ippzppppp", "dsv_keyset_census_wire", "dsv_keyset_census_mont_cols")
    add("ippzppppppzp", "dsv_keyset_census_wire_dev")
    add("i", "dsv_debug_census_lds_keys")
    return t


SIGNATURES = _signatures()
SYMBOLS = list(SIGNATURES)


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
    for name, sig in SIGNATURES.items():
        fn = getattr(L, name)  # AttributeError if a declared symbol is not exported
        fn.restype = _CTYPES[sig[0]]
        fn.argtypes = [_CTYPES[c] for c in sig[1:]]
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise DsvError("dsv error %d: %s" % (rc, load().dsv_last_error().decode()))
