"""Key sets as a key cache: the open-set verify by key value against the closed-set call and the unkeyed call, by
the share of items whose key is not registered; device-resident inputs (GPU).

    python tools/keyset_open_bench.py [--out FILE] [--log2-n 20] [--reps 21] [--k 64] [--schemes single,double,vargen]
                                      [--shares 0,1/64,1/8,1/2,1]
    python tools/keyset_open_bench.py --one SCHEME SHARE [--log2-n 20] [--reps R] [--k K]   # one cell (what the driver runs)

Each cell (scheme, miss share s) is measured in a process of its own under a time limit, profiler off: n all-valid
items in HBM, round(s * n) of them at random positions signed under valid keys that are NOT registered, the rest
under the k registered keys.  On identical items, alternating on one stream, each call timed with device events
after warm-up:
  T    KeySet.verify_open_dev (vargen: verify_vargen_open_dev): lookup, challenge hash, keyed kernel, miss list,
       unkeyed equation over the list
  A    KeySet.verify_lookup_dev on the same items (closed set: the misses get 0)
  U    dsv_verify_<scheme>_dev on all n items
  U_s  dsv_verify_<scheme>_dev on the s * n missed items alone, gathered densely beforehand
  H_s  dsv_challenge_<scheme>_dev on those same s * n items (vargen: dsv_challenge_single_dev — the scheme's
       challenge is the one-nonce-point hash of (R, m), and that export is the kernel its verify calls launch)
T's verdicts must equal U's (all 1), A's must be 1 exactly on the hits, and `misses` must equal round(s * n).
Reported per cell: medians with min and max, and the conditions
  no_cost_when_nothing_misses (s = 0)   T <= A + (max - min of A)
  cost_of_the_form                      T <= A + U_s - H_s + (max - min of T)
  faster_than_unkeyed (s <= 1/8)        T < U
"""
import argparse
import json
import os
import subprocess
import sys
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}


def measure(scheme, share, k, log2_n, reps, warmup=3):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from keyset_bench import _scalars
    from schnorr_amd import engine as E

    E.init(0)
    dev = "cuda:0"
    n = 1 << log2_n
    nmiss = int(round(Fraction(share) * n))
    # 2k keys, the first k registered: an item signed under key k + j is a valid signature that misses
    rng = np.random.default_rng(1357 + k)
    sk = _scalars(rng, 2 * k, 0x07)
    if scheme == "single":
        K0, K1 = E.public_keys(sk), None
    elif scheme == "double":
        K0, K1 = E.public_keys(sk, 0), E.public_keys(sk, 1)
    else:  # a key is the pair (PK, Gen), PK = sk * Gen: the unregistered pairs are valid keys too
        K1 = E.public_keys(_scalars(rng, 2 * k, 0x07))
        K0 = E.public_keys(sk, Gen=K1)
    missed = np.zeros(n, bool)
    missed[rng.permutation(n)[:nmiss]] = True
    idx = rng.integers(0, k, size=n) + k * missed
    m, r = _scalars(rng, n, 0x3F), _scalars(rng, n, 0x07)
    Rp = None
    if scheme == "single":
        u, R = E.sign_single(sk[idx], m, r)
    elif scheme == "double":
        u, R, Rp = E.sign_double(sk[idx], m, r)
    else:
        u, R = E.sign_vargen(sk[idx], K1[idx], m, r)
    P0, P1 = np.ascontiguousarray(K0[:k]), (np.ascontiguousarray(K1[:k]) if K1 is not None else None)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cols = [u, R] + ([Rp] if Rp is not None else []) + [K0[idx]] + ([K1[idx]] if K1 is not None else []) + [m]
    d_all = [T(c) for c in cols]
    rows = np.flatnonzero(missed)
    d_miss = [T(c[rows]) for c in cols] if nmiss else None
    ks = E.KeySet(scheme, P0, P1)
    assert (ks.key_ok() == 1).all()
    ok = {p: torch.empty(n, dtype=torch.uint8, device=dev) for p in ("T", "A", "U")}
    misses = {p: torch.zeros(1, dtype=torch.int32, device=dev) for p in ("T", "A")}
    ws = {"T": torch.empty(E.keyed_open_workspace_bytes(n), dtype=torch.uint8, device=dev),
          "A": torch.empty(E.keyed_lookup_workspace_bytes(n), dtype=torch.uint8, device=dev),
          "U": torch.empty(E.workspace_bytes(n), dtype=torch.uint8, device=dev)}
    verify = getattr(E, "verify_%s_dev" % scheme)
    verify_open = ks.verify_vargen_open_dev if scheme == "vargen" else ks.verify_open_dev
    fns = {"T": lambda: verify_open(*d_all, ok["T"], ws["T"], misses=misses["T"]),
           "A": lambda: ks.verify_lookup_dev(*d_all, ok["A"], ws["A"], misses=misses["A"]),
           "U": lambda: verify(*d_all, ok["U"], ws["U"])}
    if nmiss:
        ok_s = torch.empty(nmiss, dtype=torch.uint8, device=dev)
        ws_s = torch.empty(E.workspace_bytes(nmiss), dtype=torch.uint8, device=dev)
        c_s = torch.empty((nmiss, 32), dtype=torch.uint8, device=dev)
        npts = 2 if scheme == "double" else 1
        fns["U_s"] = lambda: verify(*d_miss, ok_s, ws_s)
        challenge = E.challenge_double_dev if scheme == "double" else E.challenge_single_dev
        fns["H_s"] = lambda: challenge(*d_miss[1:1 + npts], d_miss[-1], c_s)

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
    assert (v["U"] == 1).all(), "U: %d verdicts are not 1" % int((v["U"] != 1).sum())
    assert (v["T"] == v["U"]).all(), "T differs from U at %d items" % int((v["T"] != v["U"]).sum())
    assert (v["A"] == ~missed).all(), "A is not 1 exactly on the hits"
    assert int(misses["T"].item()) == nmiss and int(misses["A"].item()) == nmiss
    if nmiss:
        assert (ok_s.cpu().numpy() == 1).all()

    out = {"scheme": scheme, "k": k, "n": n, "reps": reps, "miss_share": str(Fraction(share)), "misses": nmiss,
           "verdicts_equal_unkeyed": True}
    for p in fns:
        out[p] = _stats(t[p])
    med = lambda p: out[p]["median_ms"] if p in out else 0.0
    spread = lambda p: out[p]["max_ms"] - out[p]["min_ms"]
    if nmiss == 0:
        out["no_cost_when_nothing_misses"] = bool(med("T") <= med("A") + spread("A"))
    out["form_bound_ms"] = round(med("A") + med("U_s") - med("H_s") + spread("T"), 4)
    out["cost_of_the_form"] = bool(med("T") <= out["form_bound_ms"])
    if Fraction(share) <= Fraction(1, 8):
        out["faster_than_unkeyed"] = bool(med("T") < med("U"))
    out["open_minus_closed_ms"] = round(med("T") - med("A"), 4)
    out["unkeyed_over_open"] = round(med("U") / med("T"), 3)
    ks.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=2, metavar=("SCHEME", "SHARE"))
    ap.add_argument("--log2-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--schemes", default="single,double,vargen")
    ap.add_argument("--shares", default="0,1/64,1/8,1/2,1")
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(measure(a.one[0], a.one[1], a.k, a.log2_n, a.reps)), flush=True)
        return
    rows = []
    for scheme in a.schemes.split(","):
        for share in a.shares.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--one", scheme, share, "--log2-n", str(a.log2_n),
                   "--reps", str(a.reps), "--k", str(a.k)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit("measurement %s s=%s failed with status %d" % (scheme, share, p.returncode))
            row = json.loads(p.stdout.strip().splitlines()[-1])
            print(json.dumps(row), flush=True)
            rows.append(row)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "w") as f:
                    json.dump({"log2_n": a.log2_n, "reps": a.reps, "k": a.k, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
