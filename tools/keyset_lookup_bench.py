"""Key sets by key value against the paths a caller has without them, device-resident inputs (GPU).

    python tools/keyset_lookup_bench.py [--out FILE] [--log2-n 20] [--reps 21] [--ks 64,16384] [--schemes single,double]
    python tools/keyset_lookup_bench.py --one SCHEME K [--log2-n 20] [--reps R]    # one measurement (what the driver runs)

Each (scheme, k) is measured in a process of its own under a time limit: n all-valid items signed under k keys,
inputs in HBM with the key COLUMNS a caller holds (the registered keys gathered per item), then on identical items,
alternating on one stream, each call timed with device events after warm-up:
  lookup_dev            KeySet.lookup_dev alone: key columns -> index column
  keyed_lookup_dev      KeySet.verify_lookup_dev: lookup, challenge hash, keyed kernel (verify by key value)
  keyed_dev             dsv_verify_<scheme>_keyed_dev with the indices computed beforehand
  unkeyed_dev           dsv_verify_<scheme>_dev on the key columns
and on the host, wall-clock, the step the lookup replaces: mapping the same n keys to indices with a dict over the
keys' bytes, and with numpy (binary search on the keys' first eight bytes, then a comparison of all bytes).
The three verdict vectors must be equal (and all 1), the looked-up indices equal to the ones the items were signed
under.  Reported: medians with the min - max spread, the lookup's share of the by-value call, the by-value call
against the unkeyed and against the keyed call, the host mapping times.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}


def measure(scheme, k, log2_n, reps, warmup=3, host_reps=3):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from keyset_bench import _signed_batch
    from schnorr_amd import engine as E

    E.init(0)
    dev = "cuda:0"
    n = 1 << log2_n
    P0, P1, idx, u, R, Rp, m = _signed_batch(E, scheme, k, n, 2468 + k)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    A, B = np.ascontiguousarray(P0[idx]), (np.ascontiguousarray(P1[idx]) if P1 is not None else None)
    du, dR, dm, di = T(u), T(R), T(m), T(idx.view(np.int32))
    pts = [dR] + ([T(Rp)] if Rp is not None else [])
    keys = [T(A)] + ([T(B)] if B is not None else [])
    ks = E.KeySet(scheme, P0, P1)
    assert (ks.key_ok() == 1).all()
    stats = ks.index_stats()
    ok = {p: torch.empty(n, dtype=torch.uint8, device=dev) for p in ("keyed_lookup_dev", "keyed_dev", "unkeyed_dev")}
    found = torch.empty(n, dtype=torch.int32, device=dev)
    misses = torch.zeros(1, dtype=torch.int32, device=dev)
    ws_l = torch.empty(E.keyed_lookup_workspace_bytes(n), dtype=torch.uint8, device=dev)
    ws_k = torch.empty(E.keyed_workspace_bytes(n), dtype=torch.uint8, device=dev)
    ws_u = torch.empty(E.workspace_bytes(n), dtype=torch.uint8, device=dev)
    fns = {"lookup_dev": lambda: ks.lookup_dev(*keys, found, misses=misses),
           "keyed_lookup_dev": lambda: ks.verify_lookup_dev(du, *pts, *keys, dm, ok["keyed_lookup_dev"], ws_l,
                                                            misses=misses),
           "keyed_dev": lambda: ks.verify_dev(du, *pts, di, dm, ok["keyed_dev"], ws_k),
           "unkeyed_dev": lambda: getattr(E, "verify_%s_dev" % scheme)(du, *pts, *keys, dm, ok["unkeyed_dev"], ws_u)}

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
    for p in v:
        assert (v[p] == 1).all(), "%s: %d verdicts are not 1" % (p, int((v[p] != 1).sum()))
    # equal keys may be registered twice (k = 16384 random keys: never in practice): the lookup gives the lowest
    first = {}
    for j in range(k):
        first.setdefault(P0[j].tobytes() + (P1[j].tobytes() if P1 is not None else b""), j)
    assert len(first) == k
    assert (found.cpu().numpy().view(np.uint32) == idx).all() and int(misses.item()) == 0

    # the host mapping this replaces: the same n keys -> indices
    rows = np.ascontiguousarray(np.hstack([A, B]) if B is not None else A)
    regs = np.ascontiguousarray(np.hstack([P0, P1]) if P1 is not None else P0)
    width = rows.shape[1]

    def by_dict():
        where = {regs[j].tobytes(): j for j in range(k)}
        flat = rows.tobytes()
        return np.fromiter((where[flat[o:o + width]] for o in range(0, n * width, width)), dtype=np.uint32, count=n)

    def by_numpy():
        head = regs[:, :8].copy().view("<u8").reshape(-1)
        order = np.argsort(head, kind="stable")
        pos = np.searchsorted(head[order], rows[:, :8].copy().view("<u8").reshape(-1))
        cand = order[np.minimum(pos, k - 1)]
        assert (regs[cand] == rows).all()
        return cand.astype(np.uint32)

    host = {}
    for name, f in (("host_dict", by_dict), ("host_numpy", by_numpy)):
        ts = []
        for _ in range(host_reps):
            t0 = time.perf_counter()
            got = f()
            ts.append((time.perf_counter() - t0) * 1e3)
            assert (got == idx).all(), name
        host[name] = _stats(ts)

    out = {"scheme": scheme, "k": k, "n": n, "reps": reps, "host_reps": host_reps, "verdicts_equal": True,
           "index": stats, "index_bytes": E.keyset_index_bytes(scheme, k), "keyset_bytes": ks.nbytes}
    for p in fns:
        out[p] = _stats(t[p])
    out.update(host)
    med = lambda p: out[p]["median_ms"]
    out["lookup_share_of_by_value_call"] = round(med("lookup_dev") / med("keyed_lookup_dev"), 4)
    out["by_value_minus_keyed_ms"] = round(med("keyed_lookup_dev") - med("keyed_dev"), 4)
    out["unkeyed_over_by_value"] = round(med("unkeyed_dev") / med("keyed_lookup_dev"), 3)
    out["by_value_faster_than_unkeyed"] = bool(med("keyed_lookup_dev") < med("unkeyed_dev"))
    out["by_value_over_keyed"] = round(med("keyed_lookup_dev") / med("keyed_dev"), 3)
    out["by_value_Mverdicts_s"] = round(n / med("keyed_lookup_dev") / 1e3, 2)
    out["host_dict_over_by_value_call"] = round(med("host_dict") / med("keyed_lookup_dev"), 1)
    out["host_numpy_over_by_value_call"] = round(med("host_numpy") / med("keyed_lookup_dev"), 1)
    ks.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=2, metavar=("SCHEME", "K"))
    ap.add_argument("--log2-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--ks", default="64,16384")
    ap.add_argument("--schemes", default="single,double")
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
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
                    json.dump({"log2_n": a.log2_n, "reps": a.reps, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
