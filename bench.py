#!/usr/bin/env python3
"""bench.py — Schnorr verifies/sec on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--log2-batch B] [--config single|mixed]
                    [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times exactly K steps, checks their verdicts against the expected
pattern and prints the headline line (`value`, `ms_per_step`).  Everything below that rides along —
per-kernel and roofline figures, the secondary schemes and input forms, the small-batch latency, the
CPU baseline and oracle samples, per-rank stage times — runs only with --full (implied by
--dump-inputs and --cpu-baseline-file).
--dump-outputs DIR writes what the last timed step computed (the verdict vector, as float32) to
DIR/verdicts.npy (with N > 1 also DIR/gathered_verdicts.npy, the all-gathered vector); the inputs
are seeded, so two builds can be compared output for output.

One "step" = one pass of the verify hot path over one batch per GPU, inputs already resident in
HBM, through the public device-pointer entry points of libdsv.so:

  --config single (default; BASELINE.json configs[1]): 2^20 single signatures per GPU through
      dsv_verify_single_dev = k_challenge (Poseidon) + k_verify_fixed_half
      ((b*u)*G + a*PK - b*R == O, halfgcd.h), cut by the library into 2^16-item sub-batches on two
      internal streams.  N > 1: every rank verifies its own shard (weak scaling) and the verdict
      bytes are all-gathered over RCCL inside the timed region.
  --config mixed (configs[4]): per GPU 2^20 items, single and double signatures interleaved by
      index parity in ONE structure of arrays; per step the kind vector is split ON THE DEVICE,
      each kind is gathered and verified by its own kernels, the two verdict vectors are
      all-gathered and scattered back into global batch order
      (schnorr_amd/distributed.py: MixedShardedVerifier).  With N > 1 the default run also reports
      this configuration as the `mixed` sub-object of its JSON line.

Launch: `python bench.py --gpus N` from a plain shell SPAWNS its N ranks itself (fresh child
processes, started before this process touches the GPU; LOCAL_RANK -> device, rendezvous on
127.0.0.1); under torch.distributed.run (RANK / WORLD_SIZE in the environment) it is one rank.

Batches are generated on the GPU by the engine's own sign kernels from the reference harness's
StdRng streams; every 16th item is corrupted, so the expected verdict vector is non-trivial; it is
checked after the timed region, and with --full at N = 1 samples are re-verified by the CPU oracle.

Prints ONE JSON line on rank 0.  `roofline` is SURVEY.md §8(d)'s figure for the dominant kernel
k_verify_fixed_half: v_mad_u64_u32 lane-operations per verdict x verdicts / the kernel's launch
duration (HIP events, one whole-batch launch on the current stream, right after the timed region),
against the measured MAD issue peak.  DESIGN.md §3 (in full: HISTORY.md §4) has the instruction model.
Riding along at N = 1: `double` (configs[2]), `vargen` (configs[3]), `mixed` (configs[4] shape),
`sign`, `ext` (projective inputs, to_hash_inputs on the device), `wire` (serialized records,
decompression on the device), `host_path` / `host_path_ext` / `wire.host` (PCIe-inclusive, never the
headline value), `verify_batch_e2e` (the named entry point over 2^20 typed objects holding the
reference's in-memory representation, conversion included; tools/verify_batch_e2e.cpp),
`small_batch` (measured first).  What is live and what is replayed from a committed PMC pass:
`roofline.pmc_source`.  With N > 1: `ranks` (per-rank step and init times; with --full also the
gather and stage times).  All of this paragraph but `ranks.ms_per_step` / `ranks.init_s` needs --full.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "Schnorr verifies/sec (single + double) at batch=2^20; 1/2/4/8 MI355X"  # BASELINE.json

# ---- work model (HISTORY.md §4; tools/isa_hist.py -> profiles/r02/isa_hist.json) ---------------
# v_mad_u64_u32 and total VALU instructions of one field operation, as hipcc emits them
MUL_MAD, MUL_ALL = 153, 189            # 81 + 72 MADs; + 36 digit / shift instructions
SQR_MAD, SQR_ALL = 117, 161            # 45 + 72 MADs; + 8 doublings + 36
WINDOWS = 65.73                        # 2-bit joint windows: mean over waves of the longest lane's count
FIXED_ADDS = 16                        # signed 16-bit windows over 253 bits
VAR_WINDOWS = 43.9                     # var-generator kernel: three ~170-bit scalars (lattice3.h), 4-bit windows
VAR_LATTICE = 22000                    # its lattice reduction: ~80 passes x ~170 + 7 exact updates x 1600


RLC_MIN = 1 << 17   # schnorr_amd/csrc/rlc.h: kRlcMinAuto — smaller groups skip the aggregate (it would be slower)
RLC_MIN_HEAVY = 1 << 14   # ... rlc_min_auto(double / var-generator), device-resident calls


def _verify_counts(chains=1):
    """(multiplications, squarings) per verdict of k_verify_fixed_half<chains>: joint table of the 11
    combinations da*PK + db*R (common.h: build_joint_table), WINDOWS x (2 doublings + 1 addition)"""
    table_m = 4 + 3 * 5 + 3 * (10 + 4)     # P, R (u*v, *2d); 2P, 2R, 2(P+R): 3M (+4S) + 2; three sum / difference pairs: 10 + 2 x 2
    table_s = 3 * 4
    dbl_m, dbl_s, add_m = 3, 4, 8           # doubling: 2uv as (u+v)^2 - (u^2+v^2)
    per_chain_m = (4 + table_m              # PK, R to Montgomery form; the table
                   + 2                      # top window: O + entry (2M + 1S)
                   + (WINDOWS - 1) * (2 * dbl_m + add_m)
                   + (FIXED_ADDS - 1) * 7 + 4)   # += (b*u)*G, mixed additions; the last only as far as the identity test needs it
    per_chain_s = table_s + 1 + (WINDOWS - 1) * 2 * dbl_s
    return chains * per_chain_m, chains * per_chain_s


def _hash_counts(double):
    """(multiplications, squarings, rows on the matrix cores, MFMA wave-instructions per wave) of
    k_challenge.  Since r02's matrix-core form (schnorr_amd/csrc/hades_mfma.h) every product with a
    constant field element — recurrence rounds, dense layers of the full rounds, start-up rows and
    state rebuild — is an int8 MFMA product; the VALU keeps the S-boxes, and per row one Barrett
    step (8 MADs + one v_mul_hi) and ~205 cheap instructions of digit packing / recombination."""
    def perm(first_const, word1_only):
        sbox = 5 * 8 + 59 - first_const
        dots5 = 5 * 8 - (4 if word1_only else 0)            # rows of the dense layer: 5 terms
        edge_terms = (7 + 9 + 11 + 13) + 5 * 10             # recurrence start-up + state rebuild
        rows = dots5 + 4 + 54 + 5
        mfma_instr = 2 * (5 * dots5 + 10 * 54 + 9 + edge_terms)   # 2 per term (one per hash tile)
        return sbox, rows, mfma_instr
    if double:   # two trips through the generic permutation body (k_hash.hip)
        a, b = perm(0, False), perm(0, True)
        sbox, rows, minstr = (a[i] + b[i] for i in range(3))
        conv = 5
    else:
        sbox, rows, minstr = perm(2, True)
        conv = 3
    return conv + 1 + sbox, 2 * sbox, rows, minstr           # +1: out of Montgomery form


MFMA_ROW_MAD, MFMA_ROW_OTHER = 9, 205


def _mads(m, s, dot_terms=0, dot_reds=0, mfma_rows=0):
    return m * MUL_MAD + s * SQR_MAD + dot_terms * 81 + dot_reds * 72 + mfma_rows * MFMA_ROW_MAD


def _valu(m, s, dot_terms=0, dot_reds=0, other=0, mfma_rows=0):
    # a limb dot product: 81 MADs per term + one operand-scanning reduction (72 MADs + 58 others); a
    # row on the matrix cores: Barrett step + digit packing / recombination
    return (m * MUL_ALL + s * SQR_ALL + dot_terms * 81 + dot_reds * 130
            + mfma_rows * (MFMA_ROW_MAD + MFMA_ROW_OTHER) + other)


# lane-instructions outside multiplications: limb-wise add / biased subtract / carry passes of the
# group law, half-gcd (~8 k since r02's alternating-role loop), recoding, conversions, identity test
VERIFY_OTHER = WINDOWS * (2 * 91 + 145) + 16 * 145 + 20 * 150 + 8000 + 1500 + 66 * 60
ALGO_BYTES = {"single": 193, "double": 321, "vargen": 257}
MAD_CYCLES = 4.12        # v_mad_u64_u32 (SGPR carry-out) per wave64, 2 waves/SIMD: profiles/r02/valu_rates.txt
N_CU, SIMD_PER_CU, CLOCK_HZ = 256, 4, 2.4e9
MAD_PEAK = N_CU * SIMD_PER_CU * CLOCK_HZ / MAD_CYCLES * 64      # lane-MADs / s
HBM_PEAK_GBS = 8000.0


def _pmc():
    """Last committed rocprofv3 PMC pass (profiles/pmc_latest.json): counters cannot be read from
    inside the timed process, so traffic / held clock are the RECORDED figures of the same
    command, not live ones.  (gfx950 under-reports FETCH_SIZE by up to 2x for wide coalesced
    reads; these are 16-B-per-lane scattered reads, uncalibrated.)"""
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_latest.json")) as f:
            return json.load(f)
    except Exception:
        return None


def _e2e_streamed(L, scheme_idx, ok, expected, n, calls=8, reps=3):
    """`calls` verify_batch* over the same typed objects with TWO batches in flight
    (verify_batch*_submit / BatchJob::wait of include/dusk_schnorr.hpp = dsv_verify_*_mont_cols_submit /
    dsv_job_wait) and, for comparison, the same calls strictly one after the other; wall time of the whole
    sequence incl. every vector<bool>, divided by the number of calls; best of `reps` sequences."""
    import ctypes

    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    ms = ctypes.c_double(0)
    res = {}
    for label, fl in (("back_to_back", 1), ("two_in_flight", 2)):
        best = None
        for _ in range(reps):
            ok[:] = 7
            rc = L.vb_e2e_run_streamed(ctypes.c_int(scheme_idx), ctypes.c_int(calls), ctypes.c_int(fl), p(ok),
                                       ctypes.byref(ms))
            if rc != 0:
                raise SystemExit("verify_batch_e2e streamed (%s): rc %d" % (label, rc))
            if (ok != expected).any():
                raise SystemExit("verify_batch_e2e streamed (%s): verdicts differ from the expected pattern" % label)
            best = ms.value / calls if best is None else min(best, ms.value / calls)
        res[label] = {"ms_per_call": best, "value": n / (best * 1e-3), "calls": calls, "in_flight": fl}
    return res


def _e2e_fast_scheme(L, scheme_idx, ok, expected):
    """verify_batch_{double,var_gen}_fast over the VALID objects of the prepared batch (the aggregate decides)"""
    import ctypes
    if not hasattr(L, "vb_e2e_run_fast_scheme"):
        return None
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    cnt, acc, ms = ctypes.c_size_t(0), ctypes.c_int(0), ctypes.c_double(0)
    mask = np.ascontiguousarray(expected)
    times = []
    for rep in range(4):
        if L.vb_e2e_run_fast_scheme(ctypes.c_int(scheme_idx), p(mask), p(ok), ctypes.byref(cnt), ctypes.byref(acc),
                                    ctypes.byref(ms)) != 0:
            raise SystemExit("verify_batch_fast (scheme %d): engine error" % scheme_idx)
        if not ok[:cnt.value].all() or bool(acc.value) != (cnt.value >= RLC_MIN):
            raise SystemExit("verify_batch_fast (scheme %d): verdicts / acceptance differ" % scheme_idx)
        if rep:
            times.append(ms.value)
    times.sort()
    return {"items": int(cnt.value), "best_ms": times[0], "value": cnt.value / (times[0] * 1e-3),
            "accepted_by_aggregate": bool(acc.value)}


def _verify_batch_e2e_double(E, bd, cores):
    """`verify_batch_double` of the C++ mirror over the double batch as typed objects (SignatureDouble
    352 B, PublicKeyDouble 320 B): six strided columns, 448 B gathered per item."""
    import ctypes

    lib_path = os.path.join(ROOT, "tools", "libvb_e2e.so")
    if not os.path.exists(lib_path):
        return None
    L = ctypes.CDLL(lib_path)
    h = {k: bd[k].cpu().numpy() for k in ("u", "R", "Rp", "PK", "PKp", "m")}
    expected = bd["expected"].cpu().numpy()
    n = h["u"].shape[0]
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    bad = L.vb_e2e_prepare_double(p(h["u"]), p(h["R"]), p(h["Rp"]), p(h["PK"]), p(h["PKp"]), p(h["m"]),
                                  ctypes.c_size_t(n), ctypes.c_int(max(1, min(cores, 16))))
    ok = np.zeros(n, dtype=np.uint8)
    ms = ctypes.c_double(0)
    try:
        times = []
        for rep in range(6):
            if L.vb_e2e_run_double(p(ok), ctypes.byref(ms)) != 0:
                raise SystemExit("verify_batch_e2e (double): engine error")
            if rep:
                times.append(ms.value)
        if (ok != expected).any():
            raise SystemExit("verify_batch_e2e (double): verdicts differ from the expected pattern")
        streamed = _e2e_streamed(L, 1, ok, expected, n)
        fast = _e2e_fast_scheme(L, 1, ok, expected)
    finally:
        L.vb_e2e_release()
    times.sort()
    return {"value": n / (times[0] * 1e-3), "unit": "verifies/s", "items": n, "best_ms": times[0],
            "median_ms": times[len(times) // 2], "objects_not_representable": int(bad),
            "streamed": streamed, "fast_accept_all_valid": fast,
            "copy_threads": E.set_host_threads(0),
            "workload": "verify_batch_double over %d typed objects (SignatureDouble 352 B, PublicKeyDouble "
                        "320 B, BlsScalar 32 B) -> vector<bool>; dsv_verify_double_mont_cols" % n}


def _verify_batch_e2e_vargen(E, bv, cores):
    """`verify_batch_var_gen` of the C++ mirror over the var-generator batch as typed objects
    (SignatureVarGen 192 B, PublicKeyVarGen 320 B): five strided columns, 352 B gathered per item."""
    import ctypes

    lib_path = os.path.join(ROOT, "tools", "libvb_e2e.so")
    if not os.path.exists(lib_path):
        return None
    L = ctypes.CDLL(lib_path)
    h = {k: bv[k].cpu().numpy() for k in ("u", "R", "PK", "Gen", "m")}
    expected = bv["expected"].cpu().numpy()
    n = h["u"].shape[0]
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    bad = L.vb_e2e_prepare_vargen(p(h["u"]), p(h["R"]), p(h["PK"]), p(h["Gen"]), p(h["m"]), ctypes.c_size_t(n),
                                  ctypes.c_int(max(1, min(cores, 16))))
    ok = np.zeros(n, dtype=np.uint8)
    ms = ctypes.c_double(0)
    try:
        times = []
        for rep in range(6):
            if L.vb_e2e_run_vargen(p(ok), ctypes.byref(ms)) != 0:
                raise SystemExit("verify_batch_e2e (var-generator): engine error")
            if rep:
                times.append(ms.value)
        if (ok != expected).any():
            raise SystemExit("verify_batch_e2e (var-generator): verdicts differ from the expected pattern")
        streamed = _e2e_streamed(L, 2, ok, expected, n)
        fast = _e2e_fast_scheme(L, 2, ok, expected)
    finally:
        L.vb_e2e_release()
    times.sort()
    return {"value": n / (times[0] * 1e-3), "unit": "verifies/s", "items": n, "best_ms": times[0],
            "median_ms": times[len(times) // 2], "objects_not_representable": int(bad),
            "streamed": streamed, "fast_accept_all_valid": fast,
            "workload": "verify_batch_var_gen over %d typed objects (SignatureVarGen 192 B, PublicKeyVarGen "
                        "320 B, BlsScalar 32 B) -> vector<bool>; dsv_verify_vargen_mont_cols" % n}


def _verify_batch_e2e(E, hu, hR, hPK, hm, expected, cores):
    """Time `verify_batch(&[Signature], &[PublicKey], &[BlsScalar]) -> Vec<bool>` of the C++ mirror
    (include/dusk_schnorr.hpp) over the whole batch as typed objects: 1 copy thread and the default
    number, best and median of 5 calls each; beside it the byte-oriented way of the r03 shim (8
    to_bytes() per signature in a serial loop) on a 2^17 subset."""
    import ctypes

    lib_path = os.path.join(ROOT, "tools", "libvb_e2e.so")
    if not os.path.exists(lib_path):
        return None
    L = ctypes.CDLL(lib_path)
    n = hu.shape[0]
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    bad = L.vb_e2e_prepare(p(hu), p(hR), p(hPK), p(hm), ctypes.c_size_t(n), ctypes.c_int(max(1, min(cores, 16))))
    ok = np.zeros(n, dtype=np.uint8)
    ms = ctypes.c_double(0)
    res = {"unit": "verifies/s", "items": n, "objects_not_representable": int(bad),
           "workload": "verify_batch over %d typed objects (Signature 192 B, PublicKey 160 B, BlsScalar "
                       "32 B; Montgomery limbs, random z per point) -> vector<bool>: field gather by the "
                       "engine's copy threads (dsv_verify_single_mont_cols), PCIe, "
                       "k_normalize_uvz + the affine path, verdict packing; no host field arithmetic" % n}
    try:
        for label, threads in (("threads_1", 1), ("threads_default", 0)):
            in_force = E.set_host_threads(threads)
            times = []
            for rep in range(6):
                if L.vb_e2e_run(p(ok), ctypes.byref(ms)) != 0:
                    raise SystemExit("verify_batch_e2e: engine error")
                if rep:
                    times.append(ms.value)
            if (ok != expected).any():
                raise SystemExit("verify_batch_e2e: verdicts differ from the expected pattern")
            times.sort()
            res[label] = {"copy_threads": in_force, "best_ms": times[0], "median_ms": times[len(times) // 2],
                          "value": n / (times[0] * 1e-3)}
        res["value"] = res["threads_default"]["value"]
        res["one_shot"] = {"best_ms": res["threads_default"]["best_ms"], "median_ms": res["threads_default"]["median_ms"],
                           "value": res["threads_default"]["value"]}
        res["streamed"] = _e2e_streamed(L, 0, ok, expected, n)
        # verify_batch_fast (SURVEY §8(f)-4 at the named entry point): the batch's VALID objects alone — the
        # aggregate decides — and the whole 1/16-tampered batch (aggregate, then the per-signature kernels)
        if hasattr(L, "vb_e2e_run_fast"):
            cnt, acc = ctypes.c_size_t(0), ctypes.c_int(0)
            fast = {}
            for label, mask in (("all_valid", np.ascontiguousarray(expected)), ("graded_workload", None)):
                times = []
                for rep in range(5):
                    if L.vb_e2e_run_fast(p(mask) if mask is not None else None, p(ok), ctypes.byref(cnt),
                                         ctypes.byref(acc), ctypes.byref(ms)) != 0:
                        raise SystemExit("verify_batch_fast: engine error")
                    want = np.ones(cnt.value, np.uint8) if mask is not None else expected
                    if (ok[:cnt.value] != want).any() or bool(acc.value) != (mask is not None and cnt.value >= RLC_MIN):
                        raise SystemExit("verify_batch_fast (%s): verdicts / acceptance differ" % label)
                    if rep:
                        times.append(ms.value)
                times.sort()
                fast[label] = {"items": int(cnt.value), "best_ms": times[0], "median_ms": times[len(times) // 2],
                               "value": cnt.value / (times[0] * 1e-3), "accepted_by_aggregate": bool(acc.value)}
            fast["all_valid"]["vs_verify_batch_one_shot"] = fast["all_valid"]["value"] / res["one_shot"]["value"]
            if hasattr(L, "vb_e2e_run_fast_streamed"):   # two calls in flight (two threads on the blocking entry point)
                E.rlc_history(0, 0)   # (the graded batch above left the device in "batches fail" mode: steady state again)
                best = None
                for rep in range(3):
                    if L.vb_e2e_run_fast_streamed(p(np.ascontiguousarray(expected)), ctypes.c_int(8), ctypes.c_int(2),
                                                  ctypes.byref(cnt), ctypes.byref(acc), ctypes.byref(ms)) != 0 \
                            or (not acc.value and cnt.value >= RLC_MIN):
                        raise SystemExit("verify_batch_fast streamed: engine error / not accepted")
                    best = ms.value if best is None else min(best, ms.value)
                fast["all_valid_two_in_flight"] = {"items": int(cnt.value), "calls": 8, "ms_per_call": best,
                                                   "value": cnt.value / (best * 1e-3)}
            res["fast_accept"] = fast
        sub = min(n, 1 << 17)
        conv, tot = ctypes.c_double(0), ctypes.c_double(0)
        if L.vb_e2e_to_bytes_path(ctypes.c_size_t(sub), p(ok), ctypes.byref(conv), ctypes.byref(tot)) != 0:
            raise SystemExit("verify_batch_e2e: to_bytes path failed")
        if (ok[:sub] != expected[:sub]).any():
            raise SystemExit("verify_batch_e2e: to_bytes path verdicts differ")
        res["to_bytes_path"] = {"items": sub, "convert_ms": conv.value, "total_ms": tot.value,
                                "value": sub / (tot.value * 1e-3),
                                "convert_only_value": sub / (conv.value * 1e-3),
                                "note": "the r03 binding: 8 to_bytes() (a Montgomery reduction each) per "
                                        "signature in one serial host loop, then dsv_verify_single_ext_multi"}
    finally:
        E.set_host_threads(0)
        L.vb_e2e_release()
    return res


DUMP_BUDGET = 64 << 20   # bytes over all files --dump-outputs writes


def _dump_outputs(dirname, arrays):
    """--dump-outputs: every array as DIR/<name>.npy in float32.  An array past its share of the budget
    is replaced by a fixed, seeded sample of its items, whose positions go to DIR/<name>_index.npy (float64)."""
    os.makedirs(dirname, exist_ok=True)
    share = DUMP_BUDGET // max(1, len(arrays))
    for name, a in arrays.items():
        a = np.asarray(a, dtype=np.float32).reshape(-1)
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(2321).choice(a.size, size=share // (4 + 8), replace=False))
            np.save(os.path.join(dirname, name + "_index.npy"), idx.astype(np.float64))
            a = a[idx]
        np.save(os.path.join(dirname, name + ".npy"), a)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _spawn_ranks(n):
    """python bench.py --gpus N from a plain shell: start N fresh rank processes (this process has
    not initialised the GPU and never will), forward rank 0's output, return the worst exit code."""
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), DSV_BENCH_SPAWNED="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        out = None if r == 0 else subprocess.DEVNULL
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:],
                                      env=env, stdout=out))
    rc = 0
    for p in procs:
        rc = max(rc, abs(p.wait()))
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log2-batch", type=int, default=20)
    ap.add_argument("--config", choices=("single", "mixed"), default="single")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-double", action="store_true", help="skip the secondary figures")
    ap.add_argument("--dump-inputs", metavar="DIR",
                    help="(implies --full) write the timed batches (single, double, var-generator) as the reference's wire records "
                         "+ the GPU verdicts into DIR: the input of rust/dusk-schnorr-gpu/src/bin/bench_ref.rs, "
                         "which times the REAL crate's pk.verify(&sig, m) over them")
    ap.add_argument("--cpu-baseline-file", metavar="JSON",
                    help="(implies --full) output of bench_ref (the real dusk-schnorr crate on this box's host cores): becomes "
                         "cpu_baseline with kind \"crate\"; the oracle's figures stay beside it as `port`")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline figure: small-batch latency, "
                         "per-kernel / roofline figures, double / var-generator / fast accept / input forms / "
                         "signing / mixed, CPU baseline and oracle samples, host paths, per-rank stage times")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the verdicts of the last timed step as DIR/<name>.npy (float32)")
    args = ap.parse_args()
    if args.dump_inputs or args.cpu_baseline_file:
        args.full = True                         # both feed on the secondary legs / the CPU baseline

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(_spawn_ranks(args.gpus))

    import torch

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("WORLD_SIZE=%d but --gpus %d" % (world, args.gpus))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP engine has no CPU fallback")
    # rehearsal knobs (one-GPU boxes): DSV_BENCH_DEVICE pins every rank to one GPU and
    # DSV_BENCH_BACKEND=gloo replaces RCCL, so the N > 1 code path can be exercised without N GPUs
    dev_index = int(os.environ.get("DSV_BENCH_DEVICE", local_rank))
    backend = os.environ.get("DSV_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(dev_index)
    dev = "cuda:%d" % dev_index

    t_init0 = time.perf_counter()
    dist = None
    # DSV_BENCH_FORCE_DIST=1: create the process group even for one rank, so that a one-GPU box
    # exercises the real RCCL collectives (all_gather / all_reduce / barrier over one rank)
    force_dist = world == 1 and os.environ.get("DSV_BENCH_FORCE_DIST") == "1"
    if force_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(_free_port()))
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
    if world > 1 or force_dist:
        import torch.distributed as dist

        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device(dev))
        else:
            dist.init_process_group(backend)

    from schnorr_amd import engine as E
    from schnorr_amd import workload as W
    from schnorr_amd.distributed import MixedShardedVerifier

    E.init(dev_index)
    torch.cuda.synchronize()
    init_s = time.perf_counter() - t_init0     # process group + engine context (two 75.5 MB tables)
    n = 1 << args.log2_batch

    multi = dist is not None

    def per_rank(x):
        """one float per rank -> {"min", "max", "argmax", "all"} (N > 1: the line must say WHICH rank lags)"""
        t = torch.tensor([x], dtype=torch.float64, device=dev)
        if multi:
            g = torch.empty(world, dtype=torch.float64, device=dev)
            dist.all_gather_into_tensor(g, t)
            t = g
        v = [float(y) for y in t.cpu()]
        return {"min": min(v), "max": max(v), "argmax": v.index(max(v)), "all": [round(y, 4) for y in v]}

    last_ranks = {}

    def sync_all():
        if multi:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(step, steps, warmup):
        """W untimed + exactly K timed steps between barrier + synchronize; max over ranks"""
        sync_all()
        for _ in range(warmup):
            step()
        sync_all()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        sync_all()
        dt = time.perf_counter() - t0
        pr = per_rank(dt / steps * 1e3)          # every rank's own clock around the same K steps
        last_ranks["ms_per_step"] = pr
        return pr["max"] * steps / 1e3           # max over ranks

    def event_pairs(k):
        return [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(k)]

    def mean_ms(pairs):
        return sum(a.elapsed_time(b) for a, b in pairs) / max(1, len(pairs))

    # ------------------------------------------------------------------ configs[4]: mixed batch
    def run_mixed(steps, warmup, keep_outputs=False):
        mb = W.gen_mixed(n, seed=2321, device=dev, first_item=rank * n)
        gk = (torch.arange(world * n, device=dev) & 1).to(torch.uint8)   # the global kind vector
        ver = MixedShardedVerifier(n, mb["n_double"], world, rank, dev, collective=multi)
        if multi:
            ver(mb, gk)                          # communicator set-up is not a step
        last = [None]

        def step_m():
            last[0] = ver(mb, gk)
        dtm = timed(step_m, steps, warmup)
        out_all = last[0]                        # the verdicts of the last timed step
        torch.cuda.synchronize()
        mine = out_all[rank * n:(rank + 1) * n]
        bad = int((mine != mb["expected"]).sum().item())
        if multi:                                # the gathered verdicts of the OTHER ranks
            exp_all = torch.empty(world * n, dtype=torch.uint8, device=dev)
            dist.all_gather_into_tensor(exp_all, mb["expected"])
            bad += int((out_all != exp_all).sum().item())
        if bad or ver.local_counts() != (n - mb["n_double"], mb["n_double"]):
            raise SystemExit("rank %d: mixed batch: %d verdicts differ / counts %r"
                             % (rank, bad, ver.local_counts()))
        outputs = {}
        if keep_outputs and rank == 0:
            outputs["verdicts"] = mine.cpu().numpy()
            if multi:
                outputs["gathered_verdicts"] = out_all.cpu().numpy()
        ranks = None
        if multi:
            ranks = {"ms_per_step": last_ranks["ms_per_step"]}
        if multi and args.full:
            prof = ver.profile(mb, gk, reps=3)   # HIP events around each stage, outside the timed region
            for k_, v_ in prof.items():
                ranks[k_] = per_rank(v_)
            # the slowest rank's stage times, side by side
            slow = ranks["ms_per_step"]["argmax"]
            ranks["slowest_rank"] = {"rank": slow, **{k_: ranks[k_]["all"][slow] for k_ in prof}}
        res = {"value": world * n * steps / dtm, "unit": "verifies/s", "ms_per_step": dtm / steps * 1e3,
               "workload": "2^%d mixed items per GPU (single on even, double on odd positions; "
                           "BASELINE configs[4] = 2^23 over 8 GPUs), device-side kind split, "
                           "two all_gathers, scatter back" % args.log2_batch,
               "n_gpus": world}
        if ranks:
            res["ranks"] = ranks
        return res, mb, outputs

    base = {
        "metric": METRIC, "unit": "verifies/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "u32x9 (29-bit limbs, u64 accumulate)",
        "world_size": world, "backend": ("rccl" if backend == "nccl" else backend) if multi else "none",
        "rccl_version": ".".join(map(str, torch.cuda.nccl.version())) if multi and backend == "nccl" else None,
        "launcher": "self-spawned" if os.environ.get("DSV_BENCH_SPAWNED") else
                    ("torch.distributed.run" if world > 1 else "single process"),
    }

    if args.config == "mixed":
        res, _, outputs = run_mixed(args.steps, args.warmup, keep_outputs=bool(args.dump_outputs))
        if args.dump_outputs and rank == 0:
            _dump_outputs(args.dump_outputs, outputs)
        if multi:
            base["ranks"] = dict(res.pop("ranks"), init_s=per_rank(init_s))
        out = dict(base, value=res["value"], ms_per_step=res["ms_per_step"],
                   data="synthetic: reference harness inputs (StdRng 2321 / 2322), GPU-signed, every "
                        "16th item of each kind corrupted",
                   config={"workload": res["workload"], "batch_per_gpu": n, "parallelism": "dp%d" % world,
                           "collective": "2 x all_gather of per-kind verdict bytes" if multi else "none"})
        if rank == 0:
            print(json.dumps(out))
        if multi:
            dist.barrier()
            dist.destroy_process_group()
        return

    # ------------------------------------------------------------------ configs[1]: single
    batch = W.gen_single(n, seed=2321, device=dev, first_item=rank * n)  # one stream, sharded
    ok = torch.zeros(n, dtype=torch.uint8, device=dev)
    ws = torch.empty(E.workspace_bytes(n), dtype=torch.uint8, device=dev)
    c = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    valid = torch.empty(n, dtype=torch.uint8, device=dev)
    gathered = torch.empty(world * n, dtype=torch.uint8, device=dev) if multi else None

    # ---- BASELINE configs[0] size through the host entry point: latency of a 1024-item call,
    # measured FIRST (a fresh process, nothing else in flight): 200 calls after 10 warm ones
    small_batch = None
    if args.full and rank == 0 and world == 1 and not args.no_double:
        sb = [batch[k][:1024].cpu().numpy() for k in ("u", "R", "PK", "m")]
        for _ in range(10):
            E.verify_single(*sb)
        lat = []
        for _ in range(200):
            t0_ = time.perf_counter()
            got_ = E.verify_single(*sb)
            lat.append((time.perf_counter() - t0_) * 1e3)
        if (got_ != batch["expected"][:1024].cpu().numpy()).any():
            raise SystemExit("small batch: verdicts differ from the expected pattern")
        lat.sort()
        med = lat[len(lat) // 2]
        small_batch = {"ms_per_call": med, "min_ms": lat[0], "median_ms": med, "p95_ms": lat[int(len(lat) * 0.95)],
                       "calls": len(lat), "value": 1024 / (med * 1e-3), "unit": "verifies/s",
                       "workload": "1024 single signatures per call, host buffers (BASELINE configs[0] "
                                   "size), eight-lanes-per-signature kernel; measured before the long legs"}

    def step():
        E.verify_single_dev(batch["u"], batch["R"], batch["PK"], batch["m"], ok, ws)
        if multi:
            dist.all_gather_into_tensor(gathered, ok)

    if multi:
        dist.all_gather_into_tensor(gathered, ok)  # RCCL connects lazily: not a step
    dt = timed(step, args.steps, args.warmup)
    ok_api = ok.clone()
    outputs = {}
    if args.dump_outputs and rank == 0:          # what the last timed step handed its caller
        outputs["verdicts"] = ok_api.cpu().numpy()
        if multi:
            outputs["gathered_verdicts"] = gathered.cpu().numpy()
    ranks = None
    if multi:
        ranks = {"ms_per_step": last_ranks["ms_per_step"], "init_s": per_rank(init_s)}
    if multi and args.full:
        # where each rank's step goes (outside the timed region: HIP events on the current stream around
        # the verify call and around the all_gather, which includes the wait for the slowest rank)
        ev_v, ev_g = event_pairs(5), event_pairs(5)
        sync_all()
        for (a, b), (c_, d_) in zip(ev_v, ev_g):
            a.record()
            E.verify_single_dev(batch["u"], batch["R"], batch["PK"], batch["m"], ok, ws)
            b.record()
            c_.record()
            dist.all_gather_into_tensor(gathered, ok)
            d_.record()
        torch.cuda.synchronize()
        ranks["verify_ms"] = per_rank(mean_ms(ev_v))
        ranks["all_gather_ms"] = per_rank(mean_ms(ev_g))

    # ---- per-kernel launch durations: one whole-batch launch each on the current stream,
    # bracketed by HIP events (outside the timed region: inside it the sub-batches of the two
    # kernels overlap on the library's internal streams, so no single launch can be bracketed)
    def event_ms(fn, reps=3):
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
               for _ in range(reps)]
        for a, b in evs:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in evs) / reps

    if args.full:
        hash_ms = event_ms(lambda: E.challenge_single_dev(batch["R"], batch["m"], c, valid))
        core_ms = event_ms(lambda: E.verify_core_dev(batch["u"], c, valid, batch["PK"], batch["R"], ok, ws))

    mism = int((ok != batch["expected"]).sum().item())
    mism_api = int((ok_api != batch["expected"]).sum().item())
    if multi:
        mine = gathered[rank * n:(rank + 1) * n]
        mism += int((mine != batch["expected"]).sum().item())
    if mism or mism_api:
        raise SystemExit("rank %d: %d / %d verdicts differ from the expected pattern"
                         % (rank, mism, mism_api))
    if outputs:
        _dump_outputs(args.dump_outputs, outputs)

    value = n * world * args.steps / dt
    out = dict(base, value=value, ms_per_step=dt / args.steps * 1e3,
               data="synthetic: reference harness inputs (StdRng::seed_from_u64(2321): sk, m, nonce "
                    "per item, restated RNG), GPU-signed, every 16th item corrupted",
               config={"workload": "2^%d single-signature batch verify per GPU (BASELINE configs[1]); "
                                   "`value` is this figure, `double` / `vargen` / `mixed` ride along with --full"
                                   % args.log2_batch,
                       "batch_per_gpu": n, "parallelism": "dp%d" % world,
                       "collective": "all_gather of verdict bytes" if multi else "none"})
    if ranks:
        out["ranks"] = ranks

    kernels = {}

    def kernel_block(name, ms, items, m, s, dt_=0, dr=0, other=0, algo_bytes=None, mfma_rows=0, mfma_instr=0):
        mads, valu = _mads(m, s, dt_, dr, mfma_rows), _valu(m, s, dt_, dr, other, mfma_rows)
        sec = ms * 1e-3
        blk = {"ms_per_launch": ms, "items": items, "mad_lane_ops_per_item": round(mads),
               "valu_lane_instr_per_item": round(valu),
               "mad_frac": mads * items / sec / MAD_PEAK,
               "valu_issue_frac": valu * items / sec / (MAD_PEAK * MAD_CYCLES / 4.05)}
        if mfma_instr:
            # v_mfma_i32_32x32x32_i8: 8 passes = 32 cycles of one SIMD's matrix core per wave instruction
            blk["mfma_wave_instr_per_wave"] = mfma_instr
            blk["mfma_pipe_frac"] = mfma_instr * (items / 64.0) * 32 / (sec * N_CU * SIMD_PER_CU * CLOCK_HZ)
        if algo_bytes:
            blk["algorithmic_GBps"] = algo_bytes * items / sec / 1e9
        kernels[name] = blk
        return blk

    if rank == 0 and args.full:
        vm, vs = _verify_counts(1)
        dom = kernel_block("k_verify_fixed_half<1>", core_ms, n, vm, vs, other=VERIFY_OTHER,
                           algo_bytes=ALGO_BYTES["single"])
        hm, hs, hrows, hmi = _hash_counts(False)
        kernel_block("k_challenge<false>", hash_ms, n, hm, hs, other=600, mfma_rows=hrows, mfma_instr=hmi)
        pmc = _pmc()
        traffic = clock = valu_busy = None
        pmc_source = None
        evidence = None
        if pmc:
            # r05: the recorded counters are valid for ONE build of the kernel — the sha256 of
            # k_verify.hip and every header it includes is stored with them; a mismatch marks every
            # replayed figure stale (the library file's own hash is informational: it is rebuilt per box)
            try:
                from schnorr_amd import build as B
                now_h = B.evidence_hashes()
            except Exception:  # noqa: BLE001
                now_h = {}
            rec_h = pmc.get("evidence") or {}
            evidence = {"recorded": rec_h, "this_build": now_h,
                        "stale": not rec_h or rec_h.get("k_verify_sources_sha256") != now_h.get("k_verify_sources_sha256"),
                        "same_library_file": bool(rec_h.get("libdsv_sha256")) and
                        rec_h.get("libdsv_sha256") == now_h.get("libdsv_sha256")}
            pmc_source = {"file": "profiles/pmc_latest.json", "live": False, "stale": evidence["stale"],
                          "captured": pmc.get("captured"), "commit": pmc.get("commit"),
                          "command": pmc.get("command"), "box_clock_held_ghz": pmc.get("clock_held_ghz"),
                          "note": "rocprofv3 --pmc passes cannot run inside the timed process: traffic and "
                                  "everything under `recorded` are REPLAYED from that file (another box of the "
                                  "same pool); frac / achieved / kernel_ms are live"}
            traffic = (pmc["FETCH_SIZE_KB"] + pmc["WRITE_SIZE_KB"]) * 1024.0 * n / pmc["batch"]
            if "SQ_INSTS_VALU" in pmc and "GRBM_GUI_ACTIVE" in pmc:
                # north_star's "VALU-busy": issue slots taken by VALU instructions in the PMC pass
                valu_busy = pmc["SQ_INSTS_VALU"] * 4.0 / (N_CU * SIMD_PER_CU * pmc["GRBM_GUI_ACTIVE"] / 8.0)
            clock = pmc.get("clock_held_ghz")
            if clock is None and "GRBM_GUI_ACTIVE" in pmc and "avg_duration_ns" in pmc:
                clock = pmc["GRBM_GUI_ACTIVE"] / 8.0 / pmc["avg_duration_ns"]
        algo = ALGO_BYTES["single"] * n
        out["roofline"] = {
            "kernel": "k_verify_fixed_half<1> (dominant: %.0f %% of a step)"
                      % (100 * core_ms / (core_ms + hash_ms)),
            "bound": "valu",       # neither HBM nor MFMA binds: integer MAD issue
            "achieved": dom["mad_lane_ops_per_item"] * n / (core_ms * 1e-3) / 1e12,
            "peak": MAD_PEAK / 1e12,
            "unit": "T lane-MAD/s",
            "frac": dom["mad_frac"],
            "mad_frac": dom["mad_frac"],
            "valu_issue_frac": dom["valu_issue_frac"],
            # what limits the kernel, in one place: the SIMDs are full (recorded.valu_busy), 31 % of what
            # they issue is not a MAD (non_mad_share: digit / shift of every column, limb-wise add / sub /
            # carry, half-gcd, recoding), and the chip holds recorded.clock_held_ghz of its 2.4 GHz at the
            # power limit: recorded.frac_at_held_clock is the live MAD fraction against the peak at the
            # clock the PMC pass saw
            "non_mad_share": 1.0 - dom["mad_lane_ops_per_item"] / float(dom["valu_lane_instr_per_item"]),
            "limit": "power (held clock) x issue slots spent on non-MAD instructions; neither HBM nor MFMA",
            "traffic": traffic,          # HBM / fabric bytes per launch, REPLAYED (pmc_source)
            "pmc_source": pmc_source,
            "evidence": evidence,
            "recorded": {"stale": evidence["stale"] if evidence else None,
                         "cache": (pmc or {}).get("cache"),
                         "traffic_ratio": traffic / algo if traffic else None,
                         "clock_held_ghz": clock,
                         "frac_at_held_clock": dom["mad_frac"] * (CLOCK_HZ / 1e9) / clock if clock else None,
                         "valu_busy": valu_busy},
            "step_mad_frac": (_mads(vm, vs) + _mads(hm, hs, mfma_rows=hrows)) * n / (dt / args.steps) / MAD_PEAK,
            "model": {"mad_cycles_per_wave_instr": MAD_CYCLES, "windows": WINDOWS,
                      "mul_sqr_per_verdict": [round(vm), round(vs)], "kernel_ms": core_ms,
                      "hash_kernel_ms": hash_ms,
                      "peak_note": "256 CU x 4 SIMD x 64 lanes x 2.4 GHz / 4.12 cycles"},
            "hbm": {"bound": "hbm", "achieved": algo / (dt / args.steps) / 1e9, "peak": HBM_PEAK_GBS,
                    "unit": "GB/s", "frac": algo / (dt / args.steps) / 1e9 / HBM_PEAK_GBS,
                    "algorithmic_bytes_per_verdict": ALGO_BYTES["single"]},
            "kernels": kernels,
        }

    # ---- secondary figures (N = 1): double (configs[2]), var-generator (configs[3]), signing
    sample_checks = {}
    if args.full and not args.no_double and world == 1:
        reps = max(1, args.steps // 2)
        bd = W.gen_double(n, seed=4242, device=dev)
        okd = torch.zeros(n, dtype=torch.uint8, device=dev)
        fd = lambda: E.verify_double_dev(bd["u"], bd["R"], bd["Rp"], bd["PK"], bd["PKp"], bd["m"], okd, ws)
        tdd = timed(fd, args.steps, args.warmup)      # the other half of the metric: the headline's protocol
        if int((okd != bd["expected"]).sum().item()):
            raise SystemExit("double-signature verdicts differ from the expected pattern")
        out["double"] = {"value": n * args.steps / tdd, "unit": "verifies/s", "steps": args.steps,
                         "warmup": args.warmup, "ms_per_step": tdd / args.steps * 1e3,
                         "workload": "2^%d double-signature batch (BASELINE configs[2]), fused "
                                     "two-equation kernel" % args.log2_batch}
        hd_ms = event_ms(lambda: E.challenge_double_dev(bd["R"], bd["Rp"], bd["m"], c, valid))
        cd_ms = event_ms(lambda: E.verify_core_double_dev(bd["u"], c, valid, bd["PK"], bd["R"],
                                                          bd["PKp"], bd["Rp"], okd, ws))
        if int((okd != bd["expected"]).sum().item()):
            raise SystemExit("fused double kernel: verdicts differ from the expected pattern")
        vm2, vs2 = _verify_counts(2)
        kernel_block("k_verify_fixed_half<2>", cd_ms, n, vm2, vs2, other=2 * VERIFY_OTHER - 9500,
                     algo_bytes=ALGO_BYTES["double"])
        hm2, hs2, hrows2, hmi2 = _hash_counts(True)
        kernel_block("k_challenge<true>", hd_ms, n, hm2, hs2, other=900, mfma_rows=hrows2, mfma_instr=hmi2)
        dom2 = kernels["k_verify_fixed_half<2>"]
        out["roofline_double"] = {
            "kernel": "k_verify_fixed_half<2> (dominant: %.0f %% of a double step)" % (100 * cd_ms / (cd_ms + hd_ms)),
            "bound": "valu", "achieved": dom2["mad_lane_ops_per_item"] * n / (cd_ms * 1e-3) / 1e12,
            "peak": MAD_PEAK / 1e12, "unit": "T lane-MAD/s", "frac": dom2["mad_frac"],
            # HBM / fabric bytes per launch of the fused kernel, REPLAYED like roofline.traffic (pmc_source)
            "traffic": ((_pmc() or {}).get("double") or {}).get("FETCH_SIZE_KB") and
                       ((_pmc()["double"]["FETCH_SIZE_KB"] + _pmc()["double"]["WRITE_SIZE_KB"]) * 1024.0 * n / _pmc()["batch"]),
            "kernel_ms": cd_ms, "hash_kernel_ms": hd_ms,
            "step_mad_frac": (_mads(vm2, vs2) + _mads(hm2, hs2, mfma_rows=hrows2)) * n / (tdd / args.steps) / MAD_PEAK,
            "hbm": {"achieved": ALGO_BYTES["double"] * n / (tdd / args.steps) / 1e9, "peak": HBM_PEAK_GBS,
                    "unit": "GB/s", "algorithmic_bytes_per_verdict": ALGO_BYTES["double"]}}
        sample_checks["double"] = (bd, okd.clone())

        nv = min(n, 1 << 18)
        bv = W.gen_vargen(nv, seed=777, device=dev)
        okv = torch.zeros(nv, dtype=torch.uint8, device=dev)
        fv = lambda: E.verify_vargen_dev(bv["u"], bv["R"], bv["PK"], bv["Gen"], bv["m"], okv, ws)
        tvv = timed(fv, reps, 1)
        if int((okv != bv["expected"]).sum().item()):
            raise SystemExit("var-generator verdicts differ from the expected pattern")
        out["vargen"] = {"value": nv * reps / tvv, "unit": "verifies/s",
                         "workload": "2^%d var-generator batch (BASELINE configs[3]), inputs from "
                                     "StdRng(777): sk, g, m, nonce per item" % (nv.bit_length() - 1)}
        var_ms = event_ms(fv)
        hv_ms = event_ms(lambda: E.challenge_single_dev(bv["R"], bv["m"], c[:nv], valid[:nv]))
        # r03 kernel (lattice3.h): x*Gen + y*PK - z*R == O, three window tables, a three-base Straus
        # chain of VAR_WINDOWS signed 4-bit windows (wave maximum, mean over waves), compare
        table = 1 + 7 * 7 + 8
        vvm = 6 + 3 * table + (2 + 2 * 8) + (VAR_WINDOWS - 1) * (4 * 3 + 3 * 8) + 2
        vvs = (VAR_WINDOWS - 1) * 4 * 4 + 1
        kernel_block("k_verify_var (whole call minus k_challenge, 2^%d items)" % (nv.bit_length() - 1),
                     max(var_ms - hv_ms, 1e-3), nv, vvm, vvs,
                     other=VAR_WINDOWS * (4 * 91 + 3 * 145) + VAR_LATTICE + 3 * 1500 + 4000,
                     algo_bytes=ALGO_BYTES["vargen"])
        sample_checks["vargen"] = (bv, okv.clone())

        # ---- random-linear-combination fast accept (opt-in entry point, NOT the headline:
        # `value` stays the per-signature path on the graded 1/16-tampered workload, where the aggregate
        # always fails).  Same verdict vectors; what is reported is the time on an ALL-VALID batch (the
        # aggregate decides) and on the graded batch (aggregate + per-signature kernels).
        wsr = torch.empty(E.rlc_workspace_bytes(n), dtype=torch.uint8, device=dev)
        okr = torch.zeros(n, dtype=torch.uint8, device=dev)
        acc_word = torch.zeros(1, dtype=torch.int32).pin_memory()   # `accepted`, written by the device: the calls only enqueue
        rlc = {"unit": "verifies/s",
               "entry_point": "dsv_verify_single_rlc_dev (enqueue-only: per-signature kernels gated by the aggregate's flag "
                              "words, verdict through a pinned word; weights from getrandom)",
               "protocol": "ms_per_call: one call, then a device synchronisation (as the per-signature figures); "
                           "pipelined: `reps` calls enqueued back to back on one stream, one synchronisation"}
        valid_b = W.gen_single(n, seed=2321, device=dev, tamper=False)
        one_b = {k: v.clone() for k, v in valid_b.items()}
        victim = (5 * n) // 8 + 77
        one_b["u"][victim, 3] ^= 0x10
        one_b["expected"][victim] = 0
        # label, batch, history the device is put into before every call (None: as the calls themselves leave it)
        # hist: (short, long) history the device is put into before every call; None: as the calls themselves leave it
        cases = (("all_valid", valid_b, None, n >= RLC_MIN),
                 ("one_bad_never_seen_before", one_b, (0, 0), False),   # a caller whose batches never failed: whole-group fallback
                 ("one_bad_first_in_a_while", one_b, (0, 128), False),  # ... failed within the last 128 calls: guarded, a second stage localises it
                 ("one_bad_in_batch", one_b, None, False),              # ... within the last 8 calls: sub-groups up front
                 ("graded_workload", batch, None, False))               # wrong items throughout: the sample skips the aggregates
        for label, b_, hist, expect_acc in cases:
            accs = []

            def f_():
                if hist is not None:
                    torch.cuda.synchronize(dev)
                    E.rlc_history(dev_index, hist[0])
                    E.rlc_history_long(dev_index, hist[1])
                E.verify_single_rlc_dev(b_["u"], b_["R"], b_["PK"], b_["m"], okr, wsr, accepted_out=acc_word)
                torch.cuda.synchronize(dev)
                accs.append(int(acc_word[0]))
            t_ = timed(f_, reps, 2)
            if int((okr != b_["expected"]).sum().item()) or any(a != int(expect_acc) for a in accs[-reps:]):
                raise SystemExit("rlc (%s): verdicts / acceptance differ from the expected pattern" % label)
            rlc[label] = {"value": n * reps / t_, "ms_per_call": t_ / reps * 1e3, "accepted_by_aggregate": expect_acc,
                          "vs_per_signature": (n * reps / t_) / value}
            if hist is None:
                tp_ = timed(lambda: E.verify_single_rlc_dev(b_["u"], b_["R"], b_["PK"], b_["m"], okr, wsr, accepted_out=acc_word), reps, 1)
                if int((okr != b_["expected"]).sum().item()) or int(acc_word[0]) != int(expect_acc):
                    raise SystemExit("rlc (%s, pipelined): verdicts / acceptance differ from the expected pattern" % label)
                rlc[label]["pipelined"] = {"value": n * reps / tp_, "ms_per_call": tp_ / reps * 1e3,
                                           "vs_per_signature": (n * reps / tp_) / value}
        # two caller streams, each with its own workspace and verdict buffer: one call's latency-bound tail
        # (~0.5 ms on 13 workgroups) runs under the next call's hash — what a caller with a stream of batches gets
        wsr2 = torch.empty(E.rlc_workspace_bytes(n), dtype=torch.uint8, device=dev)
        okr2 = torch.zeros(n, dtype=torch.uint8, device=dev)
        acc2 = torch.zeros(2, dtype=torch.int32).pin_memory()
        streams = [torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)]
        bufs = [(okr, wsr, acc2[0:1]), (okr2, wsr2, acc2[1:2])]
        turn = [0]

        def two_streams():
            k = turn[0] & 1
            turn[0] += 1
            o_, w_, a_ = bufs[k]
            E.verify_single_rlc_dev(valid_b["u"], valid_b["R"], valid_b["PK"], valid_b["m"], o_, w_, stream=streams[k],
                                    accepted_out=a_)
        E.rlc_history(dev_index, 0)
        E.rlc_history_long(dev_index, 0)
        tt_ = timed(two_streams, 2 * reps, 2)
        if not bool(okr.all()) or not bool(okr2.all()) or int(acc2[0]) != int(n >= RLC_MIN) or int(acc2[1]) != int(n >= RLC_MIN):
            raise SystemExit("rlc (two streams): verdicts / acceptance differ from the expected pattern")
        rlc["all_valid"]["two_streams"] = {"value": n * 2 * reps / tt_, "ms_per_call": tt_ / (2 * reps) * 1e3,
                                           "vs_per_signature": (n * 2 * reps / tt_) / value}
        del wsr2, okr2
        rlc["one_bad_in_2^20"] = rlc["one_bad_in_batch"] if n == 1 << 20 else None
        E.rlc_history(dev_index, 0)
        E.rlc_history_long(dev_index, 0)
        del valid_b, one_b
        # the other two schemes at their configuration sizes, all-valid batches
        for label, gen_, cols_, fn_, n_, ref_ in (
                ("double_all_valid", W.gen_double, ("u", "R", "Rp", "PK", "PKp", "m"), E.verify_double_rlc_dev, n, out["double"]["value"]),
                ("vargen_all_valid", W.gen_vargen, ("u", "R", "PK", "Gen", "m"), E.verify_vargen_rlc_dev, nv, out["vargen"]["value"])):
            b_ = gen_(n_, seed=99, device=dev, tamper=False)
            acc = []

            def f_():
                fn_(*[b_[k] for k in cols_], okr[:n_], wsr, accepted_out=acc_word)
                torch.cuda.synchronize(dev)
                acc.append(int(acc_word[0]))
            t_ = timed(f_, reps, 2)
            if not bool(okr[:n_].all()) or any(a != int(n_ >= RLC_MIN_HEAVY) for a in acc[-reps:]):
                raise SystemExit("rlc (%s): not accepted" % label)
            rlc[label] = {"items": n_, "value": n_ * reps / t_, "ms_per_call": t_ / reps * 1e3,
                          "vs_per_signature": (n_ * reps / t_) / ref_}
            del b_
        # the mixed batch (configs[4]'s shape on one GPU: n/2 singles and n/2 doubles interleaved), all valid
        bm_ = W.gen_mixed(n, seed=31, device=dev, tamper=False)
        wsm_ = torch.empty(E.mixed_rlc_workspace_bytes(n), dtype=torch.uint8, device=dev)
        wsp_ = torch.empty(E.mixed_workspace_bytes(n), dtype=torch.uint8, device=dev)
        margs = (bm_["kinds"], bm_["u"], bm_["R"], bm_["Rp"], bm_["PK"], bm_["PKp"], bm_["m"], bm_["n_double"])
        acc = []
        t_ = timed(lambda: acc.append(E.verify_mixed_rlc_dev(*margs, okr, wsm_)), reps, 1)
        if not bool(okr.all()) or any(a != (n // 2 >= RLC_MIN) for a in acc):
            raise SystemExit("rlc (mixed): not accepted")
        tp_ = timed(lambda: E.verify_mixed_dev(*margs, okr, wsp_), reps, 1)
        rlc["mixed_all_valid"] = {"items": n, "value": n * reps / t_, "ms_per_call": t_ / reps * 1e3,
                                  "vs_per_signature": tp_ / t_}
        del bm_, wsm_, wsp_
        out["rlc"] = rlc
        del wsr, okr

        # ---- projective inputs (what the reference's types hold): to_hash_inputs on the device
        zr = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev)
        zr[:, 31] = 0
        zr[:, 0] |= 1                                           # canonical, non-zero
        hz = zr.cpu().numpy()
        hh = lambda t: t.cpu().numpy()

        def projective(pt):                                     # (u z, v z, z) through the engine's own
            a = hh(pt)                                          # field multiplier (dsv_debug_fq_mul)
            return np.concatenate([E.debug_fq_mul(np.ascontiguousarray(a[:, :32]), hz),
                                   E.debug_fq_mul(np.ascontiguousarray(a[:, 32:]), hz), hz], axis=1)

        hR_uvz, hPK_uvz = projective(batch["R"]), projective(batch["PK"])
        dR_uvz, dPK_uvz = torch.from_numpy(hR_uvz).to(dev), torch.from_numpy(hPK_uvz).to(dev)
        wse = torch.empty(E.ext_workspace_bytes(n), dtype=torch.uint8, device=dev)
        oke = torch.zeros(n, dtype=torch.uint8, device=dev)
        fe_ = lambda: E.verify_single_ext_dev(batch["u"], dR_uvz, dPK_uvz, batch["m"], oke, wse)
        tee = timed(fe_, reps, 1)
        if int((oke != batch["expected"]).sum().item()):
            raise SystemExit("projective-input verdicts differ from the expected pattern")
        out["ext"] = {"value": n * reps / tee, "unit": "verifies/s",
                      "workload": "2^%d single signatures, R and PK as (u, v, z) with random z: "
                                  "dsv_verify_single_ext_dev (k_normalize_uvz: one inversion per eight "
                                  "signatures, then the affine path)" % args.log2_batch}
        # the same for the other two schemes (r06): the device-resident rate of the INPUT FORM verify_batch_double /
        # verify_batch_var_gen hand over (projective points) — what their one-shot figures are fairly compared with
        for sch_, cols_, fn_ in (("double", ("R", "Rp", "PK", "PKp"), E.verify_double_ext_dev),
                                 ("vargen", ("R", "PK", "Gen"), E.verify_vargen_ext_dev)):
            if sch_ not in sample_checks:
                continue
            b_, _ = sample_checks[sch_]
            n_ = b_["u"].shape[0]
            hz_ = hz[:n_]
            pr_ = lambda pt: torch.from_numpy(np.concatenate(
                [E.debug_fq_mul(np.ascontiguousarray(hh(pt)[:, :32]), hz_),
                 E.debug_fq_mul(np.ascontiguousarray(hh(pt)[:, 32:]), hz_), hz_], axis=1)).to(dev)
            pts_ = [pr_(b_[k]) for k in cols_]
            wse2 = torch.empty(E.ext_workspace_bytes(n_), dtype=torch.uint8, device=dev)
            fe2 = lambda: fn_(b_["u"], *pts_, b_["m"], oke[:n_], wse2)
            te2 = timed(fe2, reps, 1)
            if int((oke[:n_] != b_["expected"]).sum().item()):
                raise SystemExit("projective-input verdicts (%s) differ from the expected pattern" % sch_)
            out[sch_]["ext"] = {"value": n_ * reps / te2, "unit": "verifies/s", "items": n_,
                                "workload": "the same batch with every point as (u, v, z), random z: dsv_verify_%s_ext_dev" % sch_}
            del pts_, wse2
        del wse

        # ---- wire records (Signature 64 B + PublicKey 32 B per item): decompression on the device
        hsig = np.ascontiguousarray(np.concatenate([hh(batch["u"]), E.compress_points(hh(batch["R"]))], axis=1))
        hpk = E.compress_points(hh(batch["PK"]))
        dsig, dpk = torch.from_numpy(hsig).to(dev), torch.from_numpy(hpk).to(dev)
        wsw = torch.empty(E.wire_workspace_bytes(n), dtype=torch.uint8, device=dev)
        okw = torch.zeros(n, dtype=torch.uint8, device=dev)
        fw = lambda: E.verify_single_wire_dev(dsig, dpk, batch["m"], okw, wsw)
        tww = timed(fw, reps, 1)
        if int((okw != batch["expected"]).sum().item()):
            raise SystemExit("wire-format verdicts differ from the expected pattern")
        duv = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        dec_ms = event_ms(lambda: E.decompress_points_dev(dpk, duv, valid))
        # JubJubAffine::from_bytes per point (decode29.h): z^((t-1)/2) by sliding 4-bit windows over the
        # 222-bit constant exponent (219 + 1 squarings, 45 + 7 multiplications), three Tonelli-Shanks
        # window rounds, validation — squarings / multiplications
        dec_s, dec_m = 219 + 1 + (24 + 16 + 8) + 3 + 2, 45 + 7 + 4 + 2 + 3 * 2 + 1 + 6
        kernel_block("k_decompress (2^%d points)" % args.log2_batch, dec_ms, n, dec_m, dec_s, other=1500,
                     algo_bytes=32 + 65)
        out["wire"] = {"value": n * reps / tww, "unit": "verifies/s",
                       "workload": "2^%d single signatures as serialized records resident in HBM (64 B "
                                   "signature + 32 B key + 32 B message = 128 B per item): "
                                   "dsv_verify_single_wire_dev = 2 x k_decompress + the affine path"
                                   % args.log2_batch,
                       "k_decompress_ms_per_2^%d_points" % args.log2_batch: dec_ms,
                       "note": "two square roots per signature (~86 k MADs) on top of the 270 k of the "
                               "affine path: the wire path costs ~1.3x the affine one on the device"}
        sample_checks["wire"] = (hsig, hpk, okw.clone())
        del wsw, duv
        # ... the valid records alone through the batch fast accept (decode, then ONE aggregate): what a
        # node does with a block's serialized signatures
        keepw = torch.nonzero(batch["expected"]).flatten()
        vsig, vpk, vm = dsig[keepw].contiguous(), dpk[keepw].contiguous(), batch["m"][keepw].contiguous()
        nvw = int(keepw.numel())
        wsr = torch.empty(E.wire_rlc_workspace_bytes(nvw), dtype=torch.uint8, device=dev)
        acc = []
        fwr = lambda: acc.append(E.verify_wire_rlc_dev("single", vsig, vpk, vm, okw[:nvw], wsr))
        twr = timed(fwr, reps, 1)
        if not bool(okw[:nvw].all()) or any(a != (nvw >= RLC_MIN) for a in acc):
            raise SystemExit("wire fast accept: not accepted")
        out["wire"]["fast_accept_all_valid"] = {"items": nvw, "value": nvw * reps / twr, "ms_per_call": twr / reps * 1e3,
                                                "vs_wire_per_signature": (nvw * reps / twr) / out["wire"]["value"]}
        del wsr, vsig, vpk, vm

        # signing (the step in front of verify): R = r*G, c = H(R, m), u = r - c*sk
        sk_ = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev); sk_[:, 31] &= 0x07
        r_ = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev); r_[:, 31] &= 0x07
        su = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        sR = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        tss = timed(lambda: E.sign_single_dev(sk_, batch["m"], r_, su, sR), reps, 1)
        out["sign"] = {"value": n * reps / tss, "unit": "signatures/s",
                       "workload": "2^%d single signatures, nonces supplied" % args.log2_batch}
        del sk_, r_, su, sR
        mres, mb, _ = run_mixed(reps, 1)
        out["mixed"] = mres
        sample_checks["mixed"] = (mb, None)
        if rank == 0:
            out["roofline"]["kernels"] = kernels
    elif args.full and world > 1 and not args.no_double:
        # the multi-GPU run also measures configs[4] (2^20 mixed items per GPU), same process group
        mres, _, _ = run_mixed(max(1, args.steps // 2), 1)
        out["mixed"] = mres

    # ---- the timed batches as the reference's wire records, for the real crate's CPU loop (bench_ref.rs)
    if rank == 0 and world == 1 and args.dump_inputs:
        os.makedirs(args.dump_inputs, exist_ok=True)
        cat = lambda *a: np.ascontiguousarray(np.concatenate(a, axis=1))
        comp = lambda t: E.compress_points(t.cpu().numpy())     # JubJubAffine::to_bytes
        hn = lambda t: t.cpu().numpy()

        def dump(name, sig, pk, m, verdicts):
            for suffix, a in (("sig", sig), ("pk", pk), ("m", hn(m)), ("expected", hn(verdicts))):
                np.ascontiguousarray(a).tofile(os.path.join(args.dump_inputs, "%s_%s.bin" % (name, suffix)))
            return int(sig.shape[0])

        meta = {"single": dump("single", cat(hn(batch["u"]), comp(batch["R"])), comp(batch["PK"]), batch["m"], ok)}
        if "double" in sample_checks:
            bd, got = sample_checks["double"]
            meta["double"] = dump("double", cat(hn(bd["u"]), comp(bd["R"]), comp(bd["Rp"])),
                                  cat(comp(bd["PK"]), comp(bd["PKp"])), bd["m"], got)
        if "vargen" in sample_checks:
            bv, got = sample_checks["vargen"]
            meta["vargen"] = dump("vargen", cat(hn(bv["u"]), comp(bv["R"])), cat(comp(bv["PK"]), comp(bv["Gen"])),
                                  bv["m"], got)
        with open(os.path.join(args.dump_inputs, "meta.json"), "w") as f:
            json.dump(meta, f)
        out["dumped_inputs"] = {"dir": args.dump_inputs, "items": meta,
                                "next": "DSV_NO_LINK=1 cargo run --release --bin bench_ref -- %s" % args.dump_inputs}

    # ---- CPU baseline: the oracle (port of the reference algorithm) on the host cores
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import oracle_lib as O

        try:
            all_cores = len(os.sched_getaffinity(0))
        except AttributeError:
            all_cores = os.cpu_count() or 1
        cores = max(1, min(all_cores, 16))  # the GPU box's CPU share for one GPU
        sample = 4096 * cores
        h = lambda t, k: t[:k].cpu().numpy()
        hu, hR, hPK, hm = (h(batch[k], sample) for k in ("u", "R", "PK", "m"))
        O.verify_single(hu[:64], hR[:64], hPK[:64], hm[:64])  # warm
        tc0 = time.perf_counter()
        cpu_ok = O.verify_single(hu, hR, hPK, hm, nthreads=cores)
        tc = time.perf_counter() - tc0
        want = batch["expected"][:sample].cpu().numpy()
        if (cpu_ok != want).any() or (cpu_ok != ok[:sample].cpu().numpy()).any():
            raise SystemExit("CPU oracle disagrees with the GPU verdicts on the sample")
        one = min(sample, 2048)
        t10 = time.perf_counter()
        O.verify_single(hu[:one], hR[:one], hPK[:one], hm[:one], nthreads=1)
        t1 = time.perf_counter() - t10
        ts = time.perf_counter()
        O.keygen_sign_single(1024, 0xBEEF, nthreads=1)  # BASELINE configs[0] shape: keygen + sign
        t_sign = time.perf_counter() - ts
        cpu_model = "unknown"
        try:
            with open("/proc/cpuinfo") as f:
                cpu_model = next(l.split(":", 1)[1].strip() for l in f if l.startswith("model name"))
        except Exception:
            pass
        # every hardware thread this process may run on (the affinity count, no cap): north_star's "the reference
        # CPU verify loop timed on the same box's host cores (core count stated)" — as far as a port can state it
        # ... bounded by the container's cpu quota when there is one (cgroup v2 cpu.max / v1 cfs quota): 256 visible
        # hardware threads under a 16-cpu quota only thrash (measured: 27.7 k/s on 256 threads, 50 k/s on 16)
        quota = None
        try:
            with open("/sys/fs/cgroup/cpu.max") as f:
                q_, p_ = f.read().split()[:2]
                quota = None if q_ == "max" else max(1, int(round(int(q_) / int(p_))))
        except Exception:
            try:
                with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f, open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as g:
                    q_, p_ = int(f.read()), int(g.read())
                    quota = None if q_ <= 0 else max(1, int(round(q_ / p_)))
            except Exception:
                quota = None
        affinity_threads = all_cores
        if quota is not None:
            all_cores = min(all_cores, quota)
        all_block = None
        if all_cores > cores:
            # (2048 items per thread: a thread's start-up must not weigh — 256 items each measured LESS than 16
            #  threads did; what the figure then shows is the box's cpu quota, not its socket count)
            smp = min(n, 2048 * all_cores, 4 * sample)   # (bounded: ~10 s even where more threads do not help)
            au, aR, aPK, am = (h(batch[k], smp) for k in ("u", "R", "PK", "m"))
            ta0 = time.perf_counter()
            a_ok = O.verify_single(au, aR, aPK, am, nthreads=all_cores)
            ta = time.perf_counter() - ta0
            if (a_ok != batch["expected"][:smp].cpu().numpy()).any():
                raise SystemExit("CPU oracle (all cores) disagrees with the expected verdicts")
            all_block = {"value": smp / ta, "threads": all_cores, "items": smp, "wall_s": ta}
            del au, aR, aPK, am
        else:
            all_block = {"value": sample / tc, "threads": cores, "items": sample, "wall_s": tc,
                         "note": "the process may use no more cpus than `cores` (affinity and cpu quota): same measurement as `value`"}
        # the other two schemes' port rates, same thread count as `value`
        other = {}
        kd = 1024 * cores
        if "double" in sample_checks:
            bd_, _ = sample_checks["double"]
            cd_ = [h(bd_[x], kd) for x in ("u", "R", "Rp", "PK", "PKp", "m")]
            td0 = time.perf_counter()
            O.verify_double(*cd_, nthreads=cores)
            other["double"] = {"value": len(cd_[0]) / (time.perf_counter() - td0), "threads": cores, "items": len(cd_[0])}
        if "vargen" in sample_checks:
            bv_, _ = sample_checks["vargen"]
            cv_ = [h(bv_[x], kd) for x in ("u", "R", "PK", "Gen", "m")]
            tv0 = time.perf_counter()
            O.verify_vargen(*cv_, nthreads=cores)
            other["vargen"] = {"value": len(cv_[0]) / (time.perf_counter() - tv0), "threads": cores, "items": len(cv_[0])}
        out["cpu_baseline"] = {
            "value": sample / tc, "unit": "verifies/s", "cores": cores, "kind": "port",
            "cpu": cpu_model, "all_cores": all_block, "schemes": other,
            "host": {"affinity_threads": affinity_threads, "cpu_quota": quota},
            "sample": "first %d items of the same batch, %d threads, %.1f s wall; "
                      "1 thread: %.0f verifies/s on %d items; configs[0] shape (1024 x keygen+sign, "
                      "1 thread): %.0f /s" % (sample, cores, tc, one / t1, one, 1024 / t_sign),
        }
        # oracle samples of the secondary figures (the timed verdicts, not a re-run)
        k = 2048
        checked = []
        if "double" in sample_checks:
            bd, got = sample_checks["double"]
            w_ = O.verify_double(*(h(bd[x], k) for x in ("u", "R", "Rp", "PK", "PKp", "m")), nthreads=cores)
            if (w_ != got[:k].cpu().numpy()).any():
                raise SystemExit("CPU oracle disagrees with the GPU double verdicts on the sample")
            checked.append("double")
        if "vargen" in sample_checks:
            bv, got = sample_checks["vargen"]
            w_ = O.verify_vargen(*(h(bv[x], k) for x in ("u", "R", "PK", "Gen", "m")), nthreads=cores)
            if (w_ != got[:k].cpu().numpy()).any():
                raise SystemExit("CPU oracle disagrees with the GPU var-generator verdicts on the sample")
            checked.append("vargen")
        if "mixed" in sample_checks:
            mb, _ = sample_checks["mixed"]
            ks = mb["kinds"][:k].cpu().numpy()
            exp = mb["expected"][:k].cpu().numpy()
            cols = {x: h(mb[x], k) for x in ("u", "R", "Rp", "PK", "PKp", "m")}
            s_, d_ = ks == 0, ks == 1
            ws_ = O.verify_single(cols["u"][s_], cols["R"][s_], cols["PK"][s_], cols["m"][s_], nthreads=cores)
            wd_ = O.verify_double(*(cols[x][d_] for x in ("u", "R", "Rp", "PK", "PKp", "m")), nthreads=cores)
            if (ws_ != exp[s_]).any() or (wd_ != exp[d_]).any():
                raise SystemExit("CPU oracle disagrees with the mixed batch's expected verdicts")
            checked.append("mixed")
        if "wire" in sample_checks:
            hsig_, hpk_, got = sample_checks["wire"]
            w_ = O.verify_single_wire(hsig_[:k], hpk_[:k], h(batch["m"], k))
            if (w_ != got[:k].cpu().numpy()).any():
                raise SystemExit("CPU oracle disagrees with the GPU wire-format verdicts on the sample")
            checked.append("wire")
        out["cpu_baseline"]["oracle_samples"] = "first %d items of: single (%d), %s" % (
            k, sample, ", ".join(checked))
        if args.cpu_baseline_file:
            # the reference itself (rust/dusk-schnorr-gpu/src/bin/bench_ref.rs): pk.verify(&sig, m) of the
            # real crate over the batches --dump-inputs wrote, all cores and one thread
            with open(args.cpu_baseline_file) as f:
                ref = json.load(f)
            if ref.get("kind") != "crate" or "single" not in ref:
                raise SystemExit("--cpu-baseline-file: not a bench_ref output")
            port = out["cpu_baseline"]
            sg = ref["single"]
            out["cpu_baseline"] = {
                "value": sg["threads_all"]["value"], "unit": "verifies/s", "cores": ref.get("cores"),
                "kind": "crate", "cpu": ref.get("cpu"),
                "sample": "%s: pk.verify(&sig, m) over all %d items of the dumped single batch on %s threads "
                          "(%.1f s); 1 thread: %.0f verifies/s on %d items; verdicts differing from the GPU's: %d"
                          % (ref.get("crate"), sg["items"], sg["threads_all"].get("threads", ref.get("cores")),
                             sg["threads_all"]["seconds"], sg["threads_1"]["value"], sg["threads_1"]["items"],
                             sg["mismatches_vs_gpu"]),
                "crate": {k_: ref[k_] for k_ in ("single", "double", "vargen") if k_ in ref},
                "port": port,
            }
        # host-buffer path of the C ABI (PCIe-inclusive), never the headline value
        hu, hR, hPK, hm = (h(batch[x], n) for x in ("u", "R", "PK", "m"))
        def host_best(fn, reps=3):
            """best of `reps` whole calls after one warm call (staging buffers sized for the batch):
            a host call's time moves by +-10 % with whatever else the box's CPU share is doing"""
            got = fn()
            best = 1e9
            for _ in range(reps):
                t0_ = time.perf_counter()
                got = fn()
                best = min(best, time.perf_counter() - t0_)
            return best, got

        th, _ = host_best(lambda: E.verify_single(hu, hR, hPK, hm))
        out["host_path"] = {"value": n / th, "unit": "verifies/s",
                            "note": "dsv_verify_single on %d host-resident items incl. PCIe staging; best "
                                    "of 3 calls (so are host_path_ext and wire.host)" % n}
        if "ext" in out:
            # what the Rust / C++ verify_batch binds: projective points from host memory (256 B per
            # item instead of 192), normalised on the device
            te, got = host_best(lambda: E.verify_single_ext(hu, hR_uvz, hPK_uvz, hm))
            if (got != batch["expected"].cpu().numpy()).any():
                raise SystemExit("host projective-input verdicts differ from the expected pattern")
            out["host_path_ext"] = {"value": n / te, "unit": "verifies/s",
                                    "note": "dsv_verify_single_ext on %d host-resident items (u, v, z "
                                            "points: 256 B per item) incl. PCIe staging" % n}
            # the same with z = 1 in every point — what deserialised keys / signatures and this library's
            # own sign / keygen outputs hold: every lane's inversion is 1/1 (inv29.h answers it at once;
            # before r05 such lanes paid a failed Euclid attempt plus the whole Fermat chain)
            one = np.zeros((n, 32), dtype=np.uint8)
            one[:, 0] = 1
            z1 = lambda a: np.ascontiguousarray(np.concatenate([a, one], axis=1))
            hR_z1, hPK_z1 = z1(hR), z1(hPK)
            tz, got = host_best(lambda: E.verify_single_ext(hu, hR_z1, hPK_z1, hm))
            if (got != batch["expected"].cpu().numpy()).any():
                raise SystemExit("host projective-input (z = 1) verdicts differ from the expected pattern")
            out["host_path_ext"]["z_equals_1"] = {"value": n / tz, "unit": "verifies/s",
                                                  "note": "every point with z = 1 (affine-lifted input)"}
            del hR_z1, hPK_z1
            tw, got = host_best(lambda: E.verify_single_wire(hsig, hpk, hm))
            if (got != batch["expected"].cpu().numpy()).any():
                raise SystemExit("host wire-format verdicts differ from the expected pattern")
            out["wire"]["host"] = {"value": n / tw, "unit": "verifies/s",
                                   "note": "dsv_verify_single_wire on %d host-resident records (128 B "
                                           "per item) incl. PCIe staging" % n}
            # the valid records alone through the fast accept, from host memory (what a node does with a block)
            keep_h = np.flatnonzero(batch["expected"].cpu().numpy())
            vs, vp, vm_ = (np.ascontiguousarray(a[keep_h]) for a in (hsig, hpk, hm))
            got, acc_ = E.verify_wire_rlc("single", vs, vp, vm_)
            if not got.all() or acc_ != (len(keep_h) >= RLC_MIN):
                raise SystemExit("host wire fast accept: not accepted")
            tf, _ = host_best(lambda: E.verify_wire_rlc("single", vs, vp, vm_)[0])
            out["wire"]["host"]["fast_accept_all_valid"] = {"items": int(len(keep_h)), "value": len(keep_h) / tf,
                                                            "ms_per_call": tf * 1e3,
                                                            "vs_wire_host_per_signature": (len(keep_h) / tf) / (n / tw)}
            del vs, vp, vm_
        # ---- verify_batch END TO END from typed objects (what north_star names): the C++ mirror of the
        # reference's types holds Montgomery limbs and 160-byte projective points; conversion, PCIe,
        # engine and Vec<bool> packing are all inside the timed call (tools/verify_batch_e2e.cpp)
        e2e = _verify_batch_e2e(E, hu, hR, hPK, hm, batch["expected"].cpu().numpy(), cores)
        if e2e:
            out["verify_batch_e2e"] = e2e
            if "host_path_ext" in out:
                e2e["vs_host_path_ext"] = e2e["value"] / out["host_path_ext"]["value"]

            def ratios(d, dev_value, key):
                # one-shot and streamed (two batches in flight) against the device-resident rate of the
                # same scheme and input form, measured in this process
                d["vs_" + key] = d["value"] / dev_value
                d["streamed"]["two_in_flight"]["vs_" + key] = d["streamed"]["two_in_flight"]["value"] / dev_value
                d["streamed"]["back_to_back"]["vs_" + key] = d["streamed"]["back_to_back"]["value"] / dev_value

            if "ext" in out:  # projective input resident in HBM: what the typed objects hold
                ratios(e2e, out["ext"]["value"], "device_resident_ext")
            if "double" in sample_checks:
                e2d = _verify_batch_e2e_double(E, sample_checks["double"][0], cores)
                if e2d:
                    ratios(e2d, out["double"]["value"], "device_resident_double")
                    if "ext" in out["double"]:
                        ratios(e2d, out["double"]["ext"]["value"], "device_resident_double_ext")
                    e2e["double"] = e2d
            if "vargen" in sample_checks:
                e2v = _verify_batch_e2e_vargen(E, sample_checks["vargen"][0], cores)
                if e2v:
                    ratios(e2v, out["vargen"]["value"], "device_resident_vargen")
                    if "ext" in out["vargen"]:
                        ratios(e2v, out["vargen"]["ext"]["value"], "device_resident_vargen_ext")
                    e2e["vargen"] = e2v
            e2e["note"] = ("one-shot: a single verify_batch call on an idle GPU (ramp and tail included); "
                           "streamed.two_in_flight: a caller with a stream of batches keeps two in flight "
                           "(verify_batch_submit / BatchJob::wait), so one batch's ramp runs under the "
                           "previous one's tail — per-call time of 8 calls")
    if small_batch:
        out["small_batch"] = small_batch

    if rank == 0:
        print(json.dumps(out))
    if multi:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
