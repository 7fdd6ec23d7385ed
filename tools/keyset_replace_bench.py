"""Replacing keys of a full key set in place against rebuilding the set (GPU).

    python tools/keyset_replace_bench.py [--out FILE] [--reps 21] [--ks 64,4096] [--ms 1,16,256] [--schemes single,double]
    python tools/keyset_replace_bench.py --one SCHEME K M [--reps R]     # one measurement (what the driver runs)

Each (scheme, k, m) is measured in a process of its own under a time limit.  k + 2m random valid keys; per
repetition, alternating in the same process, each blocking call under a host clock:
  replace       (a) dsv_keyset_replace of m keys at m random distinct indices of a full set of k keys (k = capacity;
                the same set through all repetitions, the new keys alternating between two lists of m)
  rebuild       (b) dsv_keyset_create over the k final keys: what a caller had to do for the same end state
  append        (c) dsv_keyset_append of m keys to a reserved set that holds k (capacity k + m; created before the
                clock starts): the same m tables, without the quiesce and without the index rebuild
  exclusive     the part of (a) spent under the key-set lock held exclusively (the device-wide wait, the commit, the
                index rebuild), from the library's own host clock around it (dsv_debug_keyset_replace_exclusive_ns)
After the timed repetitions the replaced set and a set built at once over its final keys are compared: key_ok, and
the by-value lookup of every final and every evicted key.  For m = 1 also: the throughput of a loop of by-index
calls of 2^20 items over one second, alone and with a replace of one key every 100 ms from another thread.
The one condition: at the largest k, replace is below rebuild by more than rebuild's own
min - max spread.
"""
import argparse
import json
import os
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ITEMS = 1 << 20


def _stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}


def measure(scheme, k, m, reps, warmup=2):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from schnorr_amd import _lib
    from schnorr_amd import engine as E

    E.init(0)
    L = _lib.load()
    rng = np.random.default_rng(131 * k + m)
    sk = rng.integers(0, 256, size=(k + 2 * m, 32), dtype=np.uint8)
    sk[:, 31] &= 0x07
    P0 = E.public_keys(sk, 0)
    P1 = E.public_keys(sk, 1) if scheme == "double" else None
    cut = lambda lo, hi: [np.ascontiguousarray(P[lo:hi]) for P in (P0, P1) if P is not None]
    old, lists = cut(0, k), (cut(k, k + m), cut(k + m, k + 2 * m))
    where = np.sort(rng.permutation(k)[:m]).astype(np.uint32)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    full = E.KeySet(scheme, *old)
    final = [a.copy() for a in old]
    turn = [0]
    exclusive = []

    def replace_once():
        new = lists[turn[0] % 2]
        turn[0] += 1
        t, _ = clock(lambda: full.replace(where, *new))
        exclusive.append(L.dsv_debug_keyset_replace_exclusive_ns() / 1e6)
        for f, n in zip(final, new):
            f[where] = n
        return t

    def rebuild_once():
        t, ks = clock(lambda: E.KeySet(scheme, *final))
        ks.close()
        return t

    def append_once():
        ks = E.KeySet.reserved(scheme, k + m, *old)
        t, first = clock(lambda: ks.append(*lists[0]))
        assert first == k
        ks.close()
        return t

    fns = {"replace": replace_once, "rebuild": rebuild_once, "append": append_once}
    for _ in range(warmup):
        for f in fns.values():
            f()
    del exclusive[:]
    t = {p: [] for p in fns}
    for _ in range(reps):
        for p, f in fns.items():
            t[p].append(f())
    # the same end state
    whole = E.KeySet(scheme, *final)
    assert (full.key_ok() == whole.key_ok()).all() and (whole.key_ok() == 1).all()
    probe = [np.ascontiguousarray(np.concatenate([f, o[where]])) for f, o in zip(final, old)]
    ia, ma = full.lookup(*probe)
    ib, mb = whole.lookup(*probe)
    assert (ia == ib).all() and (ia[:k] == np.arange(k)).all() and ma == mb == m
    whole.close()

    out = {"scheme": scheme, "k": k, "m": m, "reps": reps, "end_state_equal": True}
    for p in fns:
        out[p] = _stats(t[p])
    out["exclusive"] = _stats(exclusive)
    med = lambda p: out[p]["median_ms"]
    spread = out["rebuild"]["max_ms"] - out["rebuild"]["min_ms"]
    out["rebuild_spread_ms"] = round(spread, 4)
    out["rebuild_minus_replace_ms"] = round(med("rebuild") - med("replace"), 4)
    out["replace_below_rebuild_by_more_than_its_spread"] = bool(med("rebuild") - med("replace") > spread)
    out["replace_minus_append_ms"] = round(med("replace") - med("append"), 4)
    if m == 1:
        out["throughput"] = throughput(E, torch, np, scheme, full, sk, final, where, lists)
    full.close()
    return out


def throughput(E, torch, np, scheme, ks, sk, final, where, lists, seconds=1.0, every=0.1):
    """items per second of a loop of by-index calls of 2^20 items (synchronised after each), alone and with another
    thread replacing one key every 100 ms; the items lie under keys that are not replaced"""
    k = ks.k
    rng = np.random.default_rng(5)
    keep = np.setdiff1d(np.arange(k), where)
    idx = keep[rng.integers(0, len(keep), size=N_ITEMS)].astype(np.uint32)
    msg = rng.integers(0, 256, size=(N_ITEMS, 32), dtype=np.uint8)
    msg[:, 31] &= 0x3F
    r = rng.integers(0, 256, size=(N_ITEMS, 32), dtype=np.uint8)
    r[:, 31] &= 0x07
    signed = E.sign_single(sk[idx], msg, r) if scheme == "single" else E.sign_double(sk[idx], msg, r)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    args = [dev(signed[0])] + [dev(p) for p in signed[1:]] + [dev(idx.view(np.int32)), dev(msg)]
    ok = torch.zeros(N_ITEMS, dtype=torch.uint8, device="cuda:0")
    ws = torch.empty(E.keyed_workspace_bytes(N_ITEMS), dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.Stream(device="cuda:0")

    def loop():
        torch.cuda.synchronize()
        calls, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            ks.verify_dev(*args, ok, ws, stream=st)
            st.synchronize()
            calls += 1
        return calls * N_ITEMS / (time.perf_counter() - t0)

    loop()  # warm
    assert int(ok.sum().item()) == N_ITEMS
    alone = loop()
    stop, stalls = threading.Event(), []

    def replacer():
        from schnorr_amd import _lib
        L, turn = _lib.load(), 1
        while not stop.wait(every):
            ks.replace(where, *lists[turn % 2])
            stalls.append(L.dsv_debug_keyset_replace_exclusive_ns() / 1e6)
            turn += 1

    th = threading.Thread(target=replacer)
    th.start()
    try:
        beside = loop()
    finally:
        stop.set()
        th.join()
    assert int(ok.sum().item()) == N_ITEMS
    return {"items_per_s_alone": round(alone), "items_per_s_with_replaces": round(beside), "replaces": len(stalls),
            "dip_percent": round(100.0 * (1.0 - beside / alone), 2),
            "exclusive_beside_ms": _stats(stalls) if stalls else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=3, metavar=("SCHEME", "K", "M"))
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--ks", default="64,4096")
    ap.add_argument("--ms", default="1,16,256")
    ap.add_argument("--schemes", default="single,double")
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(measure(a.one[0], int(a.one[1]), int(a.one[2]), a.reps)), flush=True)
        return
    rows = []
    ks = [int(x) for x in a.ks.split(",")]
    doc = {}
    for scheme in a.schemes.split(","):
        for k in ks:
            for m in [int(x) for x in a.ms.split(",")]:
                if m > k:  # m pairwise distinct indices below k: there is no such call
                    row = {"scheme": scheme, "k": k, "m": m, "not_applicable": "a replace takes m <= k keys"}
                else:
                    cmd = [sys.executable, os.path.abspath(__file__), "--one", scheme, str(k), str(m), "--reps",
                           str(a.reps)]
                    p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
                    if p.returncode != 0:
                        sys.stderr.write(p.stdout + p.stderr)
                        raise SystemExit("measurement %s k=%d m=%d failed with status %d" % (scheme, k, m, p.returncode))
                    row = json.loads(p.stdout.strip().splitlines()[-1])
                print(json.dumps(row), flush=True)
                rows.append(row)
                doc = {"reps": a.reps, "rows": rows,
                       "condition_holds": all(r["replace_below_rebuild_by_more_than_its_spread"] for r in rows
                                              if r["k"] == max(ks) and "not_applicable" not in r)}
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "w") as f:
                        json.dump(doc, f, indent=1)
    print(json.dumps({"condition_holds": doc.get("condition_holds")}))


if __name__ == "__main__":
    main()
