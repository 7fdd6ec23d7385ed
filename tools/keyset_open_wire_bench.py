"""The key cache for serialized records: the open-set verify by compressed key against the path a caller composes
from the existing exports and against the unkeyed wire call, by the share of items whose key is not registered;
device-resident records (GPU).

    python tools/keyset_open_wire_bench.py [--out FILE] [--log2-n 20] [--reps 21] [--k 64]
                                           [--schemes single,double,vargen] [--shares 0,1/8,1]
    python tools/keyset_open_wire_bench.py --one SCHEME SHARE [--log2-n 20] [--reps R] [--k K]   # one cell

Each cell (scheme, miss share s) is measured in a process of its own under a time limit, profiler off: n all-valid
serialized items in HBM (`Signature*::to_bytes()` and `PublicKey*::to_bytes()` records), round(s * n) of them at
random positions signed under valid keys that are NOT registered, the rest under the k registered keys.  On
identical items, alternating on one stream, each call timed with device events after warm-up:
  T    KeySet.verify_open_wire_dev: decode of the signatures, wire lookup, challenge hash, keyed kernel, miss
       list, decompression of the listed keys, unkeyed equation over the list
  C    the composed path: dsv_decompress_points_dev per key column and per nonce column (its flags accumulated),
       u copied out of the records, then KeySet.verify_open_dev (vargen: verify_vargen_open_dev) on the affine
       columns and the AND of the decode flags into its verdicts
  U    dsv_verify_<scheme>_wire_dev on all n items
  L_w  KeySet.lookup_wire_dev on the key records alone
  L_a  KeySet.lookup_dev on the decompressed key columns alone
The three verdict vectors must be equal (all 1) and `misses` must equal round(s * n) for T and C, and L_w's
indices must equal L_a's.  Reported per cell: medians with min and max, and the conditions
  faster_than_composed (s = 0)   T < C
  faster_than_unkeyed            T < U
  wire_lookup_vs_affine          L_w against L_a (the ratio; true when L_w <= L_a)
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
    else:
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
    sig = np.concatenate([u, E.compress_points(R)] + ([E.compress_points(Rp)] if Rp is not None else []), axis=1)
    krec = E.compress_points(K0) if K1 is None else np.concatenate([E.compress_points(K0), E.compress_points(K1)], axis=1)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_sig, d_pk, d_m = T(sig), T(krec[idx]), T(m)
    ns, np_ = (2 if scheme == "double" else 1), (1 if scheme == "single" else 2)
    sig_bytes, pk_bytes = 32 + 32 * ns, 32 * np_
    ks = E.KeySet.from_wire(scheme, np.ascontiguousarray(krec[:k]))
    assert (ks.key_ok() == 1).all()
    ok = {p: torch.empty(n, dtype=torch.uint8, device=dev) for p in ("T", "C", "U")}
    misses = {p: torch.zeros(1, dtype=torch.int32, device=dev) for p in ("T", "C")}
    ws = {"T": torch.empty(E.keyed_open_wire_workspace_bytes(scheme, n), dtype=torch.uint8, device=dev),
          "C": torch.empty(E.keyed_open_workspace_bytes(n), dtype=torch.uint8, device=dev),
          "U": torch.empty(E.wire_workspace_bytes(n), dtype=torch.uint8, device=dev)}
    # the composed path's own columns
    c_u = torch.empty((n, 32), dtype=torch.uint8, device=dev)
    c_pts = [torch.empty((n, 64), dtype=torch.uint8, device=dev) for _ in range(ns)]
    c_keys = [torch.empty((n, 64), dtype=torch.uint8, device=dev) for _ in range(np_)]
    c_flags = torch.empty(n, dtype=torch.uint8, device=dev)
    flat_sig, flat_pk = d_sig.view(-1), d_pk.view(-1)
    verify_open = ks.verify_vargen_open_dev if scheme == "vargen" else ks.verify_open_dev

    def composed():
        for p in range(np_):
            E.decompress_points_dev(flat_pk[32 * p:], c_keys[p], c_flags, in_stride=pk_bytes, accumulate=p > 0)
        for p in range(ns):
            E.decompress_points_dev(flat_sig[32 + 32 * p:], c_pts[p], c_flags, in_stride=sig_bytes, accumulate=True)
        c_u.copy_(d_sig[:, :32])
        verify_open(c_u, *c_pts, *c_keys, d_m, ok["C"], ws["C"], misses=misses["C"])
        ok["C"].bitwise_and_(c_flags)

    idx_w = torch.empty(n, dtype=torch.int32, device=dev)
    idx_a = torch.empty(n, dtype=torch.int32, device=dev)
    verify_wire = getattr(E, "verify_%s_wire_dev" % scheme)
    fns = {"T": lambda: ks.verify_open_wire_dev(d_sig, d_pk, d_m, ok["T"], ws["T"], misses=misses["T"]),
           "C": composed,
           "U": lambda: verify_wire(d_sig, d_pk, d_m, ok["U"], ws["U"]),
           "L_w": lambda: ks.lookup_wire_dev(d_pk, idx_w),
           "L_a": lambda: ks.lookup_dev(*c_keys, idx_a)}

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
    assert (v["C"] == v["U"]).all(), "C differs from U at %d items" % int((v["C"] != v["U"]).sum())
    assert int(misses["T"].item()) == nmiss and int(misses["C"].item()) == nmiss
    iw, ia = idx_w.cpu().numpy(), idx_a.cpu().numpy()
    assert (iw == ia).all() and ((iw == -1) == missed).all()

    out = {"scheme": scheme, "k": k, "n": n, "reps": reps, "miss_share": str(Fraction(share)), "misses": nmiss,
           "verdicts_equal": True}
    for p in fns:
        out[p] = _stats(t[p])
    med = lambda p: out[p]["median_ms"]
    if nmiss == 0:
        out["faster_than_composed"] = bool(med("T") < med("C"))
    out["faster_than_unkeyed"] = bool(med("T") < med("U"))
    out["wire_lookup_vs_affine"] = bool(med("L_w") <= med("L_a"))
    out["composed_over_new"] = round(med("C") / med("T"), 3)
    out["unkeyed_over_new"] = round(med("U") / med("T"), 3)
    out["affine_lookup_over_wire_lookup"] = round(med("L_a") / med("L_w"), 3)
    ks.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=2, metavar=("SCHEME", "SHARE"))
    ap.add_argument("--log2-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--schemes", default="single,double,vargen")
    ap.add_argument("--shares", default="0,1/8,1")
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
