"""Appending keys to a live key set against rebuilding the set (GPU).

    python tools/keyset_append_bench.py [--out FILE] [--reps 21] [--ks 64,4096] [--ms 1,16,256] [--schemes single,double]
    python tools/keyset_append_bench.py --one SCHEME K M [--reps R]     # one measurement (what the driver runs)

Each (scheme, k, m) is measured in a process of its own under a time limit.  k + m random valid keys; per
repetition, alternating in the same process, each blocking call under a host clock (all three end in a stream
synchronise inside the library):
  append        dsv_keyset_append of the last m keys to a reserved set that holds the first k (capacity k + m; the
                set is created before the clock starts and destroyed after it stops)
  rebuild       dsv_keyset_create over all k + m keys: what a caller had to do for the same end state
  create_m      dsv_keyset_create of a fresh set of the m keys alone: tables, index and one synchronise for m keys,
                all an append has to do
After the timed repetitions the grown set and the rebuilt one are compared: key_ok, and the by-value lookup of
every key.  Reported: medians with the min - max spread, and per row the two conditions of DESIGN.md §10.6:
  (a) append <= create_m + (max - min of create_m)
  (b) at the largest k with m = 1: append < rebuild
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}


def measure(scheme, k, m, reps, warmup=2):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from schnorr_amd import engine as E

    E.init(0)
    rng = np.random.default_rng(97 * k + m)
    sk = rng.integers(0, 256, size=(k + m, 32), dtype=np.uint8)
    sk[:, 31] &= 0x07
    P0 = E.public_keys(sk, 0)
    P1 = E.public_keys(sk, 1) if scheme == "double" else None
    cut = lambda P, lo, hi: np.ascontiguousarray(P[lo:hi]) if P is not None else None
    old, new = (cut(P0, 0, k), cut(P1, 0, k)), (cut(P0, k, k + m), cut(P1, k, k + m))

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    def append_once(keep=False):
        ks = E.KeySet.reserved(scheme, k + m, *old)
        t, first = clock(lambda: ks.append(*[p for p in new if p is not None]))
        assert first == k and ks.k == k + m
        if keep:
            return t, ks
        ks.close()
        return t, None

    def create_once(a, b, keep=False):
        t, ks = clock(lambda: E.KeySet(scheme, a, b))
        if keep:
            return t, ks
        ks.close()
        return t, None

    fns = {"append": append_once, "rebuild": lambda: create_once(P0, P1), "create_m": lambda: create_once(*new)}
    for _ in range(warmup):
        for f in fns.values():
            f()
    t = {p: [] for p in fns}
    for _ in range(reps):
        for p, f in fns.items():
            t[p].append(f()[0])
    # the same end state
    _, grown = append_once(keep=True)
    _, whole = create_once(P0, P1, keep=True)
    assert (grown.key_ok() == whole.key_ok()).all() and (whole.key_ok() == 1).all()
    cols = [P0] + ([P1] if P1 is not None else [])
    ig, mg = grown.lookup(*cols)
    iw, mw = whole.lookup(*cols)
    assert (ig == iw).all() and (iw == np.arange(k + m)).all() and mg == mw == 0
    grown.close()
    whole.close()

    out = {"scheme": scheme, "k": k, "m": m, "reps": reps, "end_state_equal": True,
           "keyset_bytes": E.keyset_bytes(scheme, k + m)}
    for p in fns:
        out[p] = _stats(t[p])
    med = lambda p: out[p]["median_ms"]
    spread = out["create_m"]["max_ms"] - out["create_m"]["min_ms"]
    out["append_minus_create_m_ms"] = round(med("append") - med("create_m"), 4)
    out["create_m_spread_ms"] = round(spread, 4)
    out["a_append_within_create_m_plus_spread"] = bool(med("append") <= med("create_m") + spread)
    out["rebuild_over_append"] = round(med("rebuild") / med("append"), 2)
    out["append_faster_than_rebuild"] = bool(med("append") < med("rebuild"))
    return out


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
    for scheme in a.schemes.split(","):
        for k in ks:
            for m in [int(x) for x in a.ms.split(",")]:
                cmd = [sys.executable, os.path.abspath(__file__), "--one", scheme, str(k), str(m), "--reps", str(a.reps)]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
                if p.returncode != 0:
                    sys.stderr.write(p.stdout + p.stderr)
                    raise SystemExit("measurement %s k=%d m=%d failed with status %d" % (scheme, k, m, p.returncode))
                row = json.loads(p.stdout.strip().splitlines()[-1])
                print(json.dumps(row), flush=True)
                rows.append(row)
                doc = {"reps": a.reps, "rows": rows,
                       "condition_a_holds": all(r["a_append_within_create_m_plus_spread"] for r in rows),
                       "condition_b_holds": all(r["append_faster_than_rebuild"] for r in rows
                                                if r["k"] == max(ks) and r["m"] == 1)}
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    with open(a.out, "w") as f:
                        json.dump(doc, f, indent=1)
    print(json.dumps({"condition_a_holds": doc["condition_a_holds"], "condition_b_holds": doc["condition_b_holds"]}))


if __name__ == "__main__":
    main()
