"""Registered key sets against the unkeyed verify entry points, device-resident inputs (GPU).

    python tools/keyset_bench.py [--out FILE] [--log2-n 20] [--reps 21] [--ks 1,64,4096,16384]
    python tools/keyset_bench.py --one SCHEME K [--reps R]      # one measurement (what the driver runs)
    python tools/keyset_bench.py --rlc [--out FILE] [--log2-ns 18,20] [--ks ...] [--workloads valid,wrong_h8,wrong_h0]
    python tools/keyset_bench.py --soak 10000000 [--out FILE]   # keyed fast accept against the keyed per-signature path
    python tools/keyset_bench.py --wire [--out FILE] [--log2-ns 20,14] [--ks 1,64,4096]   # the keyed wire form
    python tools/keyset_bench.py --mont [--out FILE] [--log2-ns 20,14] [--ks 1,64,4096]   # the keyed typed-object form
    python tools/keyset_bench.py --soak-mont 10000000 [--out FILE]   # typed keyed forms against the affine keyed path

Each (scheme, k) is measured in a process of its own: n items signed under k keys, inputs in HBM, then
dsv_verify_<scheme>_keyed_dev and dsv_verify_<scheme>_dev on the gathered keys alternate on one stream,
each timed with device events after warm-up; the verdict vectors must be equal.  Reported: the median of
the reps per path, the ratio, and the key-set build time per key (dsv_keyset_create, host arrays in,
blocking).  Kernel times: run one measurement under `rocprofv3 --kernel-trace --stats -- python ...`.

--rlc: the keyed fast accept (KeySet.verify_rlc_dev) against the keyed per-signature path (KeySet.verify_dev)
and the unkeyed fast accept (verify_*_rlc_dev on the gathered keys), on identical device-resident inputs, for
three workloads: all valid; one wrong item with the history counters at 8 (a caller whose batches fail now and
then: sub-groups); one wrong item with the counters at 0 (the first wrong batch after a run of valid ones).
The counters are set before every timed call; all three paths must return the same verdict vector.
--wire: serialized signatures against a key set (KeySet.verify_wire_dev), per (scheme, k, n) in one process on
identical seeded inputs, the paths alternating, each call timed with device events: (a) the keyed wire call,
(b) the keyed call on the pre-decoded columns, (c) dsv_decompress_points_dev alone on the batch's nonce points,
(d) the unkeyed wire call with the gathered key records; (a) must equal (b) AND the decode flags, and (d).  At
k = 64 and the largest n the host forms follow, on pageable arrays, wall-clock: the keyed wire host call, the
keyed host call on decoded columns, the unkeyed wire host call.  Medians with the min - max spread beside them.
--mont: the reference's in-memory objects against a key set (KeySet.verify_mont_dev), per (scheme, k, n) in one
process on identical seeded inputs (a signed block of <= 2^14 items, every point re-represented with a random z,
converted to Montgomery limbs with Python integers and tiled on the device), the paths alternating, each call
timed with device events: (a) the keyed typed call, (b) the keyed call on the pre-normalised affine columns,
(c) the unkeyed typed call (dsv_verify_*_mont_dev) with the keys gathered per item, (d) the unkeyed affine call;
all four verdict vectors must be equal.  D = a - b is what the typed form costs a keyed call, D0 = c - d what it
costs an unkeyed one (which normalises 2 / 4 / 3 points where the keyed form normalises 1 / 2 / 1).  At k = 64
and the largest n the host forms follow on records laid out like the Rust structs in pageable memory,
wall-clock: the keyed typed call, the unkeyed typed call on the same objects with the keys carried per item,
two keyed jobs in flight, the blocking affine keyed call on pre-converted arrays; and the constructors
(dsv_keyset_create_mont_cols against dsv_keyset_create) at k = 64 and 16384.
--soak: calls of 2^20 items (a fresh set of wrong items, none to many, and forced sub-groups per call) through
both keyed paths; reports how many verdicts differ.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMES = ("single", "double", "vargen")


def _scalars(rng, n, top_mask):
    import numpy as np

    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= top_mask
    return s


def measure(scheme, k, log2_n, reps, warmup=3):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from schnorr_amd import engine as E

    E.init(0)
    dev = "cuda:0"
    n = 1 << log2_n
    rng = np.random.default_rng(1234 + k)
    sk = _scalars(rng, k, 0x07)
    gen = None
    if scheme == "single":
        P0, P1 = E.public_keys(sk), None
    elif scheme == "double":
        P0, P1 = E.public_keys(sk, 0), E.public_keys(sk, 1)
    else:
        gen = E.public_keys(_scalars(rng, k, 0x07))
        P0, P1 = E.public_keys(sk, Gen=gen), gen
    idx = rng.integers(0, k, size=n).astype(np.uint32)
    m, r = _scalars(rng, n, 0x3F), _scalars(rng, n, 0x07)
    Rp = None
    if scheme == "single":
        u, R = E.sign_single(sk[idx], m, r)
    elif scheme == "double":
        u, R, Rp = E.sign_double(sk[idx], m, r)
    else:
        u, R = E.sign_vargen(sk[idx], gen[idx], m, r)
    u[::16, 0] ^= 1  # some false verdicts
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    du, dR, dm, di = T(u), T(R), T(m), T(idx.view(np.int32))
    dRp = T(Rp) if Rp is not None else None
    g0, g1 = T(P0[idx]), (T(P1[idx]) if P1 is not None else None)
    torch.cuda.synchronize()

    t0 = time.perf_counter()
    ks = E.KeySet(scheme, P0, P1)
    build_s = time.perf_counter() - t0
    assert (ks.key_ok() == 1).all()

    ok_k = torch.empty(n, dtype=torch.uint8, device=dev)
    ok_u = torch.empty(n, dtype=torch.uint8, device=dev)
    ws_k = torch.empty(E.keyed_workspace_bytes(n), dtype=torch.uint8, device=dev)
    ws_u = torch.empty(E.workspace_bytes(n), dtype=torch.uint8, device=dev)
    keyed_args = (du, dR) + ((dRp,) if dRp is not None else ()) + (di, dm, ok_k, ws_k)

    def keyed():
        ks.verify_dev(*keyed_args)

    def unkeyed():
        if scheme == "single":
            E.verify_single_dev(du, dR, g0, dm, ok_u, ws_u)
        elif scheme == "double":
            E.verify_double_dev(du, dR, dRp, g0, g1, dm, ok_u, ws_u)
        else:
            E.verify_vargen_dev(du, dR, g0, g1, dm, ok_u, ws_u)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for _ in range(warmup):
        keyed()
        unkeyed()
    torch.cuda.synchronize()
    tk, tu = [], []
    for _ in range(reps):
        tk.append(timed(keyed))
        tu.append(timed(unkeyed))
    torch.cuda.synchronize()
    vk, vu = ok_k.cpu().numpy(), ok_u.cpu().numpy()
    assert (vk == vu).all(), "keyed and unkeyed verdicts differ at %d items" % int((vk != vu).sum())
    assert 0.9 < vk.mean() < 0.95, vk.mean()
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"scheme": scheme, "k": k, "n": n, "reps": reps, "keyed_ms": round(med(tk), 4),
           "unkeyed_ms": round(med(tu), 4), "speedup": round(med(tu) / med(tk), 3),
           "keyed_Mverdicts_s": round(n / med(tk) / 1e3, 2), "unkeyed_Mverdicts_s": round(n / med(tu) / 1e3, 2),
           "build_us_per_key": round(build_s / k * 1e6, 2), "keyset_bytes": ks.nbytes, "verdicts_equal": True}
    ks.close()
    return out


def _signed_batch(E, scheme, k, n, seed):
    import numpy as np

    rng = np.random.default_rng(seed)
    sk = _scalars(rng, k, 0x07)
    gen = None
    if scheme == "single":
        P0, P1 = E.public_keys(sk), None
    elif scheme == "double":
        P0, P1 = E.public_keys(sk, 0), E.public_keys(sk, 1)
    else:
        gen = E.public_keys(_scalars(rng, k, 0x07))
        P0, P1 = E.public_keys(sk, Gen=gen), gen
    idx = rng.integers(0, k, size=n).astype(np.uint32)
    m, r = _scalars(rng, n, 0x3F), _scalars(rng, n, 0x07)
    Rp = None
    if scheme == "single":
        u, R = E.sign_single(sk[idx], m, r)
    elif scheme == "double":
        u, R, Rp = E.sign_double(sk[idx], m, r)
    else:
        u, R = E.sign_vargen(sk[idx], gen[idx], m, r)
    return P0, P1, idx, u, R, Rp, m


def measure_rlc(scheme, k, log2_n, reps, workload, warmup=2, bits=0):
    """median ms of keyed per-signature, keyed fast accept and unkeyed fast accept on one workload (bits: the
    keyed fast accept's window bits, 0 = automatic)"""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from schnorr_amd import engine as E

    E.init(0)
    dev = "cuda:0"
    n = 1 << log2_n
    P0, P1, idx, u, R, Rp, m = _signed_batch(E, scheme, k, n, 4321 + k)
    if workload != "valid":
        u[n // 3, 0] ^= 1  # one wrong signature
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    du, dR, dm, di = T(u), T(R), T(m), T(idx.view(np.int32))
    dRp = T(Rp) if Rp is not None else None
    g0, g1 = T(P0[idx]), (T(P1[idx]) if P1 is not None else None)
    ks = E.KeySet(scheme, P0, P1)
    ok = {p: torch.empty(n, dtype=torch.uint8, device=dev) for p in ("keyed", "keyed_rlc", "rlc")}
    ws_k = torch.empty(E.keyed_workspace_bytes(n), dtype=torch.uint8, device=dev)
    ws_kr = torch.empty(E.keyed_rlc_workspace_bytes(n, k, bits), dtype=torch.uint8, device=dev)
    ws_r = torch.empty(E.rlc_workspace_bytes(n), dtype=torch.uint8, device=dev)
    acc = {p: torch.zeros(1, dtype=torch.int32, device=dev) for p in ("keyed_rlc", "rlc")}
    items = (du, dR) + ((dRp,) if dRp is not None else ()) + (di, dm)
    hist = {"valid": None, "wrong_h8": 8, "wrong_h0": 0}[workload]
    torch.cuda.synchronize()

    def keyed():
        ks.verify_dev(*items, ok["keyed"], ws_k)

    def keyed_rlc():
        if hist is not None:
            E.keyed_rlc_history(0, hist)
        ks.verify_rlc_dev(*items, ok["keyed_rlc"], ws_kr, window_bits=bits, accepted_out=acc["keyed_rlc"])

    def rlc():
        if hist is not None:
            E.rlc_history(0, hist)
            E.rlc_history_long(0, 0)  # (no guarded second stage: the keyed path has none)
        a = dict(accepted_out=acc["rlc"])
        if scheme == "single":
            E.verify_single_rlc_dev(du, dR, g0, dm, ok["rlc"], ws_r, **a)
        elif scheme == "double":
            E.verify_double_rlc_dev(du, dR, dRp, g0, g1, dm, ok["rlc"], ws_r, **a)
        else:
            E.verify_vargen_rlc_dev(du, dR, g0, g1, dm, ok["rlc"], ws_r, **a)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    fns = {"keyed": keyed, "keyed_rlc": keyed_rlc, "rlc": rlc}
    for _ in range(warmup):
        for f in fns.values():
            f()
    t = {p: [] for p in fns}
    for _ in range(reps):
        for p, f in fns.items():
            t[p].append(timed(f))
    torch.cuda.synchronize()
    v = {p: o.cpu().numpy() for p, o in ok.items()}
    assert (v["keyed"] == v["keyed_rlc"]).all(), "keyed fast accept differs at %d items" % int((v["keyed"] != v["keyed_rlc"]).sum())
    assert (v["keyed"] == v["rlc"]).all(), "unkeyed fast accept differs at %d items" % int((v["keyed"] != v["rlc"]).sum())
    med = lambda x: sorted(x)[len(x) // 2]
    out = {"scheme": scheme, "k": k, "n": n, "workload": workload, "reps": reps, "window_bits": bits}
    for p in fns:
        out[p + "_ms"] = round(med(t[p]), 4)
    out["keyed_rlc_vs_keyed"] = round(med(t["keyed"]) / med(t["keyed_rlc"]), 3)
    out["keyed_rlc_vs_rlc"] = round(med(t["rlc"]) / med(t["keyed_rlc"]), 3)
    out["accepted"] = {p: int(a.item()) for p, a in acc.items()}
    out["verdicts_equal"] = True
    ks.close()
    return out


def _stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}


def measure_wire(scheme, k, log2_n, reps, host, warmup=3, host_reps=7):
    """the keyed wire form against the paths a caller has without it (module docstring: --wire)"""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from schnorr_amd import engine as E

    E.init(0)
    dev = "cuda:0"
    n = 1 << log2_n
    P0, P1, idx, u, R, Rp, m = _signed_batch(E, scheme, k, n, 8765 + k)
    u[::16, 0] ^= 1  # some false verdicts
    nonce = [R] + ([Rp] if Rp is not None else [])
    sig = np.ascontiguousarray(np.concatenate([u] + [E.compress_points(p) for p in nonce], axis=1))
    rec = E.compress_points(P0) if P1 is None else np.hstack([E.compress_points(P0), E.compress_points(P1)])
    pk = np.ascontiguousarray(rec[idx])
    sig[7::4096, 32 + 31] = 0x7F  # a few undecodable nonce points (v >= q)
    sb = sig.shape[1]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dsig, dpk, dm, di = T(sig), T(pk), T(m), T(idx.view(np.int32))
    ks = E.KeySet(scheme, P0, P1)
    ok = {p: torch.empty(n, dtype=torch.uint8, device=dev) for p in "abcd"}
    cols = [torch.empty((n, 64), dtype=torch.uint8, device=dev) for _ in nonce]
    du = dsig[:, :32].contiguous()
    ws_a = torch.empty(E.keyed_wire_workspace_bytes(scheme, n), dtype=torch.uint8, device=dev)
    ws_b = torch.empty(E.keyed_workspace_bytes(n), dtype=torch.uint8, device=dev)
    ws_d = torch.empty(E.wire_workspace_bytes(n), dtype=torch.uint8, device=dev)
    flat = dsig.reshape(-1)

    def a():
        ks.verify_wire_dev(dsig, di, dm, ok["a"], ws_a)

    def c():
        for j, out in enumerate(cols):
            E.decompress_points_dev(flat[32 + 32 * j:], out, ok["c"], in_stride=sb, accumulate=j > 0)

    def b():
        ks.verify_dev(du, *cols, di, dm, ok["b"], ws_b)

    def d():
        getattr(E, "verify_%s_wire_dev" % scheme)(dsig, dpk, dm, ok["d"], ws_d)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    fns = {"a": a, "c": c, "b": b, "d": d}  # (c before b: b reads the columns c wrote)
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    t = {p: [] for p in fns}
    for _ in range(reps):
        for p, f in fns.items():
            t[p].append(timed(f))
    torch.cuda.synchronize()
    v = {p: o.cpu().numpy() for p, o in ok.items()}
    assert (v["a"] == (v["b"] & v["c"])).all(), "keyed wire differs from the composed path at %d items" % int((v["a"] != (v["b"] & v["c"])).sum())
    assert (v["a"] == v["d"]).all(), "keyed wire differs from the unkeyed wire call at %d items" % int((v["a"] != v["d"]).sum())
    assert (v["c"] == 0).sum() == len(range(7, n, 4096)) and 0.9 < v["a"].mean() < 0.95, v["a"].mean()
    names = {"a": "keyed_wire_dev", "b": "keyed_dev_predecoded", "c": "decompress_dev", "d": "wire_dev"}
    out = {"scheme": scheme, "k": k, "n": n, "reps": reps, "verdicts_equal": True}
    for p in "abcd":
        out[names[p]] = _stats(t[p])
    med = lambda p: out[names[p]]["median_ms"]
    out["a_minus_b_minus_c_ms"] = round(med("a") - med("b") - med("c"), 4)
    out["a_spread_ms"] = round(out[names["a"]]["max_ms"] - out[names["a"]]["min_ms"], 4)
    out["relation_a_le_b_plus_c_holds"] = bool(out["a_minus_b_minus_c_ms"] <= out["a_spread_ms"])
    out["wire_dev_over_keyed_wire_dev"] = round(med("d") / med("a"), 3)
    out["keyed_wire_dev_Mverdicts_s"] = round(n / med("a") / 1e3, 2)
    if host:
        uv = [o.cpu().numpy() for o in cols]
        want = v["a"]
        uh = np.ascontiguousarray(sig[:, :32])
        paths = {"keyed_wire_host": lambda: ks.verify_wire(sig, idx, m),
                 "keyed_host_predecoded": lambda: ks.verify(uh, *uv, idx, m) & v["c"],
                 "wire_host": lambda: getattr(E, "verify_%s_wire" % scheme)(sig, pk, m)}
        th = {p: [] for p in paths}
        for p, f in paths.items():
            assert (f() == want).all(), p  # (warm-up)
        for _ in range(host_reps):
            for p, f in paths.items():
                t0 = time.perf_counter()
                got = f()
                th[p].append((time.perf_counter() - t0) * 1e3)
                assert (got == want).all(), p
        for p in paths:
            out[p] = _stats(th[p])
            out[p]["Mverdicts_s"] = round(n / out[p]["median_ms"] / 1e3, 2)
        out["host_reps"] = host_reps
        out["keyed_wire_host_over_dev_rate"] = round(med("a") / out["keyed_wire_host"]["median_ms"], 3)
    ks.close()
    return out


def _mont_block(E, scheme, k, block, seed):
    """a signed block in both forms: canonical affine columns and Montgomery limbs of the same values with a
    random z per point (tests/mont_cases.py: Python integers), for the items and for the k keys"""
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import harness as H
    import mont_cases as MC
    import pymodel as M

    P0, P1, idx, u, R, Rp, m = _signed_batch(E, scheme, k, block, seed)
    rng = np.random.default_rng(seed + 1)
    limbs = lambda pts: MC.to_limbs_py(H.projective(pts, rng)[0], M.Q)
    aff = {"u": u, "R": R, "Rp": Rp, "m": m, "P0": P0, "P1": P1}
    typed = {"u": MC.to_limbs_py(u, M.R_ORDER), "m": MC.to_limbs_py(m, M.Q), "R": limbs(R),
             "Rp": limbs(Rp) if Rp is not None else None, "P0": limbs(P0), "P1": limbs(P1) if P1 is not None else None}
    return idx, aff, typed


def _records(scheme, typed, keys_of_item, n):
    """the Rust structs in pageable memory: n signature records, n key records (the keys carried per item, what
    the unkeyed typed call reads) -> (column views of the signatures, of the per-item keys)"""
    import numpy as np

    import mont_cases as MC

    pts = [typed["R"]] + ([typed["Rp"]] if scheme == "double" else [])
    sigs, pks, msgs, views = MC.as_records(scheme, [typed["u"]] + pts + keys_of_item + [typed["m"]])
    block = len(msgs)
    times = -(-n // block)
    if times > 1:
        sigs, pks, msgs = np.tile(sigs, times)[:n], np.tile(pks, times)[:n], np.tile(msgs, (times, 1))[:n]
    raw = lambda rec: rec.view(np.uint8).reshape(len(rec), rec.dtype.itemsize)
    field = lambda rec, path: (lambda off: raw(rec)[:, off:off + 96])(
        sum(t.fields[f][1] for t, f in path))
    st, pt = sigs.dtype, pks.dtype
    sig_views = [raw(sigs)[:, :32], field(sigs, [(st, "R")])] + ([field(sigs, [(st, "R_prime")])] if scheme == "double" else [])
    key_views = [field(pks, [(pt, nm)]) for nm in pt.names]
    return sigs, pks, np.ascontiguousarray(msgs), sig_views, key_views


def measure_mont(scheme, k, log2_n, reps, host, warmup=3, host_reps=7):
    """the keyed typed-object form against the paths a caller has without it (module docstring: --mont)"""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from schnorr_amd import engine as E

    E.init(0)
    dev = "cuda:0"
    n = 1 << log2_n
    block = min(n, 1 << 14)
    idx, aff, typed = _mont_block(E, scheme, k, block, 4321 + k)
    idx = idx.copy()
    idx[::16] = (idx[::16] + 1) % k if k > 1 else k  # some false verdicts: another key (one key: out of range)
    times = n // block
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tile = lambda a: T(a).repeat(*([times] + [1] * (a.ndim - 1))) if times > 1 else T(a)
    two = scheme != "single"
    pts_t = [tile(typed["R"])] + ([tile(typed["Rp"])] if scheme == "double" else [])
    pts_a = [tile(aff["R"])] + ([tile(aff["Rp"])] if scheme == "double" else [])
    keys_t = [tile(typed["P0"][idx % k])] + ([tile(typed["P1"][idx % k])] if two else [])
    keys_a = [tile(aff["P0"][idx % k])] + ([tile(aff["P1"][idx % k])] if two else [])
    un_t, un_a = pts_t + keys_t, pts_a + keys_a  # canonical order: the signature's points, then the key's
    di = tile(idx.view(np.int32))
    ut, mt, ua, ma = tile(typed["u"]), tile(typed["m"]), tile(aff["u"]), tile(aff["m"])
    ks = E.KeySet.from_mont_cols(scheme, [typed["P0"]] + ([typed["P1"]] if two else []))
    ok = {p: torch.empty(n, dtype=torch.uint8, device=dev) for p in "abcd"}
    ws = {"a": E.keyed_mont_workspace_bytes(scheme, n), "b": E.keyed_workspace_bytes(n), "c": E.mont_workspace_bytes(n),
          "d": E.workspace_bytes(n)}
    ws = {p: torch.empty(b, dtype=torch.uint8, device=dev) for p, b in ws.items()}
    fns = {"a": lambda: ks.verify_mont_dev(ut, *pts_t, di, mt, ok["a"], ws["a"]),
           "b": lambda: ks.verify_dev(ua, *pts_a, di, ma, ok["b"], ws["b"]),
           "c": lambda: getattr(E, "verify_%s_mont_dev" % scheme)(ut, *un_t, mt, ok["c"], ws["c"]),
           "d": lambda: getattr(E, "verify_%s_dev" % scheme)(ua, *un_a, ma, ok["d"], ws["d"])}

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    t = {p: [] for p in fns}
    for _ in range(reps):
        for p, f in fns.items():
            t[p].append(timed(f))
    torch.cuda.synchronize()
    v = {p: o.cpu().numpy() for p, o in ok.items()}
    in_range = np.tile(idx, times) < k
    for p in "bcd":
        same = v["a"] == v[p] if p == "b" else (v["a"][in_range] == v[p][in_range])  # (c, d read key idx % k)
        assert same.all(), "path %s differs from the keyed typed call at %d items" % (p, int((~same).sum()))
    assert 0.9 < v["a"].mean() < 0.95 or k == 1, v["a"].mean()
    names = {"a": "keyed_mont_dev", "b": "keyed_dev_prenormalised", "c": "mont_dev", "d": "affine_dev"}
    out = {"scheme": scheme, "k": k, "n": n, "reps": reps, "verdicts_equal": True}
    for p in "abcd":
        out[names[p]] = _stats(t[p])
    med = lambda p: out[names[p]]["median_ms"]
    out["D_ms"] = round(med("a") - med("b"), 4)
    out["D0_ms"] = round(med("c") - med("d"), 4)
    out["a_spread_ms"] = round(out[names["a"]]["max_ms"] - out[names["a"]]["min_ms"], 4)
    out["relation_D_le_D0_plus_spread_holds"] = bool(out["D_ms"] <= out["D0_ms"] + out["a_spread_ms"])
    out["mont_dev_over_keyed_mont_dev"] = round(med("c") / med("a"), 3)
    out["keyed_mont_dev_Mverdicts_s"] = round(n / med("a") / 1e3, 2)
    if host:
        want = v["a"]
        idx_n = np.tile(idx, times)
        per_item = [typed["P0"][idx % k]] + ([typed["P1"][idx % k]] if two else [])
        sigs, pks, msgs, sig_views, key_views = _records(scheme, typed, per_item, n)
        keyed_cols = sig_views + [idx_n, msgs]
        unkeyed_cols = sig_views + key_views + [msgs]
        host_aff = [np.tile(a, (times, 1)) for a in [aff["u"], aff["R"]] + ([aff["Rp"]] if scheme == "double" else [])]
        m_aff = np.tile(aff["m"], (times, 1))

        def two_jobs():
            j0, j1 = ks.submit_mont_cols(keyed_cols), ks.submit_mont_cols(keyed_cols)
            a0, a1 = j0.wait(), j1.wait()
            assert (a0 == a1).all()
            return a0

        paths = {"keyed_mont_cols": lambda: ks.verify_mont_cols(keyed_cols),
                 "mont_cols": lambda: E.verify_mont_cols(scheme, unkeyed_cols),
                 "keyed_mont_cols_two_jobs": two_jobs,
                 "keyed_affine_host": lambda: ks.verify(*host_aff, idx_n, m_aff)}
        th = {p: [] for p in paths}
        for p, f in paths.items():
            got = f()  # (warm-up)
            assert (got[in_range] == want[in_range]).all(), p
        for _ in range(host_reps):
            for p, f in paths.items():
                t0 = time.perf_counter()
                got = f()
                th[p].append((time.perf_counter() - t0) * 1e3)
                assert (got[in_range] == want[in_range]).all(), p
        for p in paths:
            out[p] = _stats(th[p])
            items = 2 * n if p.endswith("two_jobs") else n
            out[p]["Mverdicts_s"] = round(items / out[p]["median_ms"] / 1e3, 2)
        out["host_reps"] = host_reps
        un = out["mont_cols"]
        out["keyed_host_minus_unkeyed_host_ms"] = round(out["keyed_mont_cols"]["median_ms"] - un["median_ms"], 4)
        out["unkeyed_host_spread_ms"] = round(un["max_ms"] - un["min_ms"], 4)
        out["relation_keyed_host_not_slower_holds"] = bool(
            out["keyed_host_minus_unkeyed_host_ms"] <= out["unkeyed_host_spread_ms"])
        out["mont_cols_over_keyed_mont_cols"] = round(un["median_ms"] / out["keyed_mont_cols"]["median_ms"], 3)
    ks.close()
    return out


def measure_mont_build(kk, reps=3):
    """dsv_keyset_create_mont_cols against dsv_keyset_create (single scheme): blocking wall-clock per set"""
    import numpy as np

    sys.path.insert(0, ROOT)
    from schnorr_amd import engine as E

    E.init(0)
    _, aff, typed = _mont_block(E, "single", kk, 64, 777 + kk)
    out = {"k": kk, "reps": reps}
    for name, make in (("create_mont_cols", lambda: E.KeySet.from_mont_cols("single", [typed["P0"]])),
                       ("create", lambda: E.KeySet("single", aff["P0"]))):
        ts = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            ks = make()
            ts.append((time.perf_counter() - t0) * 1e3)
            assert (ks.key_ok() == 1).all()
            ks.close()
        out[name] = _stats(ts[1:])
        out[name]["us_per_key"] = round(out[name]["median_ms"] * 1e3 / kk, 2)
    return out


def soak_mont(total, log2_n=20, k=64, seed=2026):
    """the typed keyed _dev and host forms against the affine keyed _dev call over `total` verdicts, the three
    schemes in turn, fresh wrong items (another key's index, indices out of range) per call"""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from schnorr_amd import engine as E

    E.init(0)
    dev = "cuda:0"
    n = 1 << log2_n
    block = 1 << 14
    times = n // block
    rng = np.random.default_rng(seed)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tile = lambda a: T(a).repeat(*([times] + [1] * (a.ndim - 1)))
    done, calls, differ_dev, differ_host, zeros = 0, 0, 0, 0, 0
    sets = {}
    while done < total:
        scheme = SCHEMES[calls % 3]
        if scheme not in sets:
            idx, aff, typed = _mont_block(E, scheme, k, block, seed + calls)
            two = scheme != "single"
            pts = ["R"] + (["Rp"] if scheme == "double" else [])
            sets[scheme] = {
                "ks": E.KeySet.from_mont_cols(scheme, [typed["P0"]] + ([typed["P1"]] if two else [])),
                "idx": np.tile(idx, times),
                "typed": [tile(typed["u"])] + [tile(typed[p]) for p in pts] + [tile(typed["m"])],
                "aff": [tile(aff["u"])] + [tile(aff[p]) for p in pts] + [tile(aff["m"])],
                "host": [np.tile(typed["u"], (times, 1))] + [np.tile(typed[p], (times, 1)) for p in pts] +
                        [np.tile(typed["m"], (times, 1))]}
        s = sets[scheme]
        ks = s["ks"]
        idx = s["idx"].copy()
        wrong = int(rng.choice([0, 1, 3, 1000, 100000]))
        at = rng.integers(0, n, size=wrong)
        idx[at] = (idx[at] + 1 + rng.integers(0, k - 1, size=wrong)) % k
        far = rng.integers(0, n, size=int(rng.choice([0, 2, 50])))
        idx[far] = rng.choice([k, k + 1, (1 << 32) - 1], size=len(far))
        di = T(idx.view(np.int32))
        ok_t = torch.empty(n, dtype=torch.uint8, device=dev)
        ok_a = torch.empty(n, dtype=torch.uint8, device=dev)
        ks.verify_mont_dev(*s["typed"][:-1], di, s["typed"][-1], ok_t,
                           torch.empty(E.keyed_mont_workspace_bytes(scheme, n), dtype=torch.uint8, device=dev))
        ks.verify_dev(*s["aff"][:-1], di, s["aff"][-1], ok_a,
                      torch.empty(E.keyed_workspace_bytes(n), dtype=torch.uint8, device=dev))
        host = ks.verify_mont_cols(s["host"][:-1] + [idx, s["host"][-1]])
        torch.cuda.synchronize()
        ref = ok_a.cpu().numpy()
        differ_dev += int((ok_t.cpu().numpy() != ref).sum())
        differ_host += int((host != ref).sum())
        zeros += int((ref == 0).sum())
        done += n
        calls += 1
    for v in sets.values():
        v["ks"].close()
    return {"verdicts": done, "calls": calls, "false_verdicts": zeros, "differ_dev": differ_dev,
            "differ_host": differ_host, "k": k, "n": n}


def soak(total, log2_n=20, k=64, seed=99):
    """keyed fast accept vs keyed per-signature verdicts over `total` verdicts, all three schemes in turn"""
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from schnorr_amd import engine as E

    E.init(0)
    dev = "cuda:0"
    n = 1 << log2_n
    rng = np.random.default_rng(seed)
    done, differ, calls, accepted = 0, 0, 0, 0
    sets = {}
    while done < total:
        scheme = SCHEMES[calls % 3]
        if scheme not in sets:
            P0, P1, idx, u, R, Rp, m = _signed_batch(E, scheme, k, n, seed + calls)
            sets[scheme] = (E.KeySet(scheme, P0, P1), idx, u, R, Rp, m)
        ks, idx, u, R, Rp, m = sets[scheme]
        uu = u.copy()
        wrong = rng.choice([0, 0, 1, 3, 1000])
        uu[rng.integers(0, n, size=wrong), 0] ^= 1
        E.rlc_subgroups(int(rng.choice([0, 0, 1, 2, 16])))
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        items = (T(uu), T(R)) + ((T(Rp),) if Rp is not None else ()) + (T(idx.view(np.int32)), T(m))
        ok_a = torch.empty(n, dtype=torch.uint8, device=dev)
        ok_b = torch.empty(n, dtype=torch.uint8, device=dev)
        ks.verify_dev(*items, ok_a, torch.empty(E.keyed_workspace_bytes(n), dtype=torch.uint8, device=dev))
        acc = ks.verify_rlc_dev(*items, ok_b, torch.empty(E.keyed_rlc_workspace_bytes(n, k), dtype=torch.uint8, device=dev))
        torch.cuda.synchronize()
        differ += int((ok_a != ok_b).sum().item())
        accepted += int(acc)
        done += n
        calls += 1
    E.rlc_subgroups(0)
    for v in sets.values():
        v[0].close()
    return {"verdicts": done, "calls": calls, "accepted_calls": accepted, "differ": differ, "k": k, "n": n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=2, metavar=("SCHEME", "K"))
    ap.add_argument("--log2-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--ks", default="1,64,4096,16384")
    ap.add_argument("--schemes", default=",".join(SCHEMES))
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--rlc", action="store_true")
    ap.add_argument("--one-rlc", nargs=4, metavar=("SCHEME", "K", "LOG2N", "WORKLOAD"))
    ap.add_argument("--log2-ns", default="18,20")
    ap.add_argument("--workloads", default="valid,wrong_h8,wrong_h0")
    ap.add_argument("--soak", type=int)
    ap.add_argument("--wire", action="store_true")
    ap.add_argument("--one-wire", nargs=4, metavar=("SCHEME", "K", "LOG2N", "HOST"))
    ap.add_argument("--bits", type=int, default=0)
    ap.add_argument("--mont", action="store_true")
    ap.add_argument("--one-mont", nargs=4, metavar=("SCHEME", "K", "LOG2N", "HOST"))
    ap.add_argument("--one-mont-build", type=int, metavar="K")
    ap.add_argument("--build-ks", default="64,16384")
    ap.add_argument("--soak-mont", type=int)
    a = ap.parse_args()
    if a.soak_mont:
        row = soak_mont(a.soak_mont)
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(row, f, indent=1)
        return
    if a.one_mont:
        s, k, l2, host = a.one_mont
        print(json.dumps(measure_mont(s, int(k), int(l2), a.reps, host == "1")), flush=True)
        return
    if a.one_mont_build:
        print(json.dumps(measure_mont_build(a.one_mont_build)), flush=True)
        return
    if a.mont:
        rows, builds = [], []
        ks = [int(x) for x in (a.ks if a.ks != "1,64,4096,16384" else "1,64,4096").split(",")]
        l2s = [int(x) for x in (a.log2_ns if a.log2_ns != "18,20" else "20,14").split(",")]
        jobs = [("row", ["--one-mont", scheme, str(k), str(l2), "1" if (k == 64 and l2 == max(l2s)) else "0"])
                for scheme in a.schemes.split(",") for l2 in l2s for k in ks]
        jobs += [("build", ["--one-mont-build", x]) for x in a.build_ks.split(",") if x]
        for kind, args in jobs:
            cmd = [sys.executable, os.path.abspath(__file__)] + args + ["--reps", str(a.reps)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit("measurement %s failed with status %d" % (" ".join(args), p.returncode))
            row = json.loads(p.stdout.strip().splitlines()[-1])
            print(json.dumps(row), flush=True)
            (rows if kind == "row" else builds).append(row)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    json.dump({"reps": a.reps, "rows": rows, "set_construction": builds}, f, indent=1)
        return
    if a.soak:
        row = soak(a.soak)
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(row, f, indent=1)
        return
    if a.one_wire:
        s, k, l2, host = a.one_wire
        print(json.dumps(measure_wire(s, int(k), int(l2), a.reps, host == "1")), flush=True)
        return
    if a.wire:
        rows = []
        ks = [int(x) for x in (a.ks if a.ks != "1,64,4096,16384" else "1,64,4096").split(",")]
        l2s = [int(x) for x in (a.log2_ns if a.log2_ns != "18,20" else "20,14").split(",")]
        for scheme in a.schemes.split(","):
            for l2 in l2s:
                for k in ks:
                    host = "1" if (k == 64 and l2 == max(l2s)) else "0"
                    cmd = [sys.executable, os.path.abspath(__file__), "--one-wire", scheme, str(k), str(l2), host,
                           "--reps", str(a.reps)]
                    p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
                    if p.returncode != 0:
                        sys.stderr.write(p.stdout + p.stderr)
                        raise SystemExit("measurement %s k=%d 2^%d failed with status %d" % (scheme, k, l2, p.returncode))
                    row = json.loads(p.stdout.strip().splitlines()[-1])
                    print(json.dumps(row), flush=True)
                    rows.append(row)
                    if a.out:
                        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                        with open(a.out, "w") as f:
                            json.dump({"reps": a.reps, "rows": rows}, f, indent=1)
        return
    if a.one_rlc:
        s, k, l2, w = a.one_rlc
        print(json.dumps(measure_rlc(s, int(k), int(l2), a.reps, w, bits=a.bits)), flush=True)
        return
    if a.rlc:
        rows = []
        for scheme in a.schemes.split(","):
            for l2 in [int(x) for x in a.log2_ns.split(",")]:
                for k in [int(x) for x in a.ks.split(",")]:
                    for w in a.workloads.split(","):
                        cmd = [sys.executable, os.path.abspath(__file__), "--one-rlc", scheme, str(k), str(l2), w,
                               "--reps", str(a.reps)]
                        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
                        if p.returncode != 0:
                            sys.stderr.write(p.stdout + p.stderr)
                            raise SystemExit("measurement %s k=%d 2^%d %s failed with status %d" % (scheme, k, l2, w, p.returncode))
                        row = json.loads(p.stdout.strip().splitlines()[-1])
                        print(json.dumps(row), flush=True)
                        rows.append(row)
                        if a.out:
                            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                            with open(a.out, "w") as f:
                                json.dump({"rows": rows}, f, indent=1)
        return
    if a.one:
        print(json.dumps(measure(a.one[0], int(a.one[1]), a.log2_n, a.reps)), flush=True)
        return
    rows = []
    for scheme in a.schemes.split(","):
        for k in [int(x) for x in a.ks.split(",")]:
            cmd = [sys.executable, os.path.abspath(__file__), "--one", scheme, str(k), "--log2-n", str(a.log2_n),
                   "--reps", str(a.reps)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit("measurement %s k=%d failed with status %d" % (scheme, k, p.returncode))
            row = json.loads(p.stdout.strip().splitlines()[-1])
            print(json.dumps(row), flush=True)
            rows.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"log2_n": a.log2_n, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
