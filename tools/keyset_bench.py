"""Registered key sets against the unkeyed verify entry points, device-resident inputs (GPU).

    python tools/keyset_bench.py [--out FILE] [--log2-n 20] [--reps 21] [--ks 1,64,4096,16384]
    python tools/keyset_bench.py --one SCHEME K [--reps R]      # one measurement (what the driver runs)
    python tools/keyset_bench.py --rlc [--out FILE] [--log2-ns 18,20] [--ks ...] [--workloads valid,wrong_h8,wrong_h0]
    python tools/keyset_bench.py --soak 10000000 [--out FILE]   # keyed fast accept against the keyed per-signature path
    python tools/keyset_bench.py --wire [--out FILE] [--log2-ns 20,14] [--ks 1,64,4096]   # the keyed wire form

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
    a = ap.parse_args()
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
