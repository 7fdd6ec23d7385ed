"""The key cache for typed objects: the open-set verify over verify_batch's arguments against what
a typed-object caller runs today, by the share of items whose key is not registered (GPU).

    python tools/keyset_open_mont_bench.py [--out FILE] [--log2-ns 14,20] [--ks 64,4096] [--shares 0,1/64,1/8,1]
                                           [--schemes single,double,vargen] [--reps 21] [--host] [--soak VERDICTS]
    python tools/keyset_open_mont_bench.py --one SCHEME K LOG2N SHARE   # one device cell (the fused front, or
                                                                       # DSV_OPEN_MONT_FUSED=0: the two launches)
    python tools/keyset_open_mont_bench.py --one-host SCHEME SHARE      # one host cell: 2^20 records, k = 64

Each cell is measured in processes of its own, profiler off: a block of 2^12 all-valid items signed under 2k keys, of
which the first k are registered; round(s * block) items at random positions are under unregistered keys; every key
is presented with a fresh random z; the block is tiled to n on the device.  On identical items, alternating on one
stream, each call timed with device events after warm-up (median of --reps with min and max):
  T    KeySet.verify_open_mont_dev (dsv_verify_keyed_open_mont_dev)
  T'   the same call in a process started with DSV_OPEN_MONT_FUSED=0 (the knob is read by dsv_init), beside U as
       that process's reference
  U    dsv_verify_<scheme>_mont_dev on all n items: what the caller runs today
  K    KeySet.verify_mont_dev with the true indices (s = 0 only): the floor
  A    dsv_verify_<scheme>_dev on the normalised columns: D0 = U - A is what normalising every point costs
The verdict vectors of T, U (and K) must be equal and `misses` must be as constructed.  Conditions per cell, judged
against U's own max - min: cache_pays (s < 1) T < U by more than U's spread; cost_of_form (s = 0) T - K <= D0 + spread.
--host: 2^20 records laid out like the Rust structs in pageable memory, wall-clock median (min - max) of 7 alternating
calls of verify_open_mont_cols, verify_mont_cols, (s = 0) verify_mont_cols by index, and two open jobs in flight; again
once per value of the knob (with DSV_PIPE_TRACE=1 in the environment, --one-host labels the library's per-call
breakdown on stderr by path).  --soak: T against U on the device and the host form against U, fresh blocks per round,
the three schemes in turn; the count of differing verdicts must be 0.
"""
import argparse
import json
import os
import subprocess
import sys
import time
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
BLOCK = 1 << 12


def _stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}


def _sided_block(E, scheme, k, share, seed):
    """one block: 2k keys of which the first k get registered, every item's key drawn on the wanted side —
    registered (index < k) or not (k .. 2k - 1) —, signed, and re-represented as Montgomery limbs with a fresh random
    z per point (tests/mont_cases.py: Python integers)"""
    import numpy as np

    import keyset_bench as KB

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import harness as H
    import mont_cases as MC
    import pymodel as M

    nmiss = int(round(Fraction(share) * BLOCK))
    rng = np.random.default_rng(seed)
    sk = KB._scalars(rng, 2 * k, 0x07)
    gen = None
    if scheme == "single":
        P0, P1 = E.public_keys(sk), None
    elif scheme == "double":
        P0, P1 = E.public_keys(sk, 0), E.public_keys(sk, 1)
    else:
        gen = E.public_keys(KB._scalars(rng, 2 * k, 0x07))
        P0, P1 = E.public_keys(sk, Gen=gen), gen
    missed = np.zeros(BLOCK, bool)
    missed[rng.permutation(BLOCK)[:nmiss]] = True
    idx = (rng.integers(0, k, size=BLOCK) + k * missed).astype(np.uint32)
    m, r = KB._scalars(rng, BLOCK, 0x3F), KB._scalars(rng, BLOCK, 0x07)
    Rp = None
    if scheme == "single":
        u, R = E.sign_single(sk[idx], m, r)
    elif scheme == "double":
        u, R, Rp = E.sign_double(sk[idx], m, r)
    else:
        u, R = E.sign_vargen(sk[idx], gen[idx], m, r)
    limbs = lambda pts: MC.to_limbs_py(H.projective(pts, rng)[0], M.Q)
    pts = [R] + ([Rp] if Rp is not None else [])
    keys = [P0[idx]] + ([P1[idx]] if P1 is not None else [])
    return {"aff": [u] + pts + keys + [m],
            "typed": [MC.to_limbs_py(u, M.R_ORDER)] + [limbs(p) for p in pts + keys] + [MC.to_limbs_py(m, M.Q)],
            "reg": [np.ascontiguousarray(P0[:k])] + ([np.ascontiguousarray(P1[:k])] if P1 is not None else []),
            "idx": idx, "missed": missed, "nsig": len(pts), "nkey": len(keys)}


def measure(scheme, k, log2_n, share, reps, warmup=3):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from schnorr_amd import engine as E

    fused = os.environ.get("DSV_OPEN_MONT_FUSED", "1") != "0"
    E.init(0)
    dev = "cuda:0"
    n = 1 << log2_n
    b = _sided_block(E, scheme, k, share, 2468 + k)
    block = min(n, BLOCK)
    times = n // block
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a[:block])).to(dev)
    tile = lambda a: T(a).repeat(*([times] + [1] * (a.ndim - 1))).contiguous() if times > 1 else T(a)
    typed, aff = [tile(c) for c in b["typed"]], [tile(c) for c in b["aff"]]
    ns = b["nsig"]
    nmiss = int(b["missed"][:block].sum()) * times
    ks = E.KeySet(scheme, *b["reg"])
    assert (ks.key_ok() == 1).all()
    names = ["T", "U"] + (["K", "A"] if fused else [])
    if nmiss:
        names = [p for p in names if p != "K"]
    ok = {p: torch.empty(n, dtype=torch.uint8, device=dev) for p in names}
    misses = torch.zeros(1, dtype=torch.int32, device=dev)
    sizes = {"T": E.keyed_open_mont_workspace_bytes(scheme, n), "U": E.mont_workspace_bytes(n),
             "K": E.keyed_mont_workspace_bytes(scheme, n), "A": E.workspace_bytes(n)}
    ws = {p: torch.empty(sizes[p], dtype=torch.uint8, device=dev) for p in names}
    di = tile(b["idx"].view(np.int32))
    fns = {"T": lambda: ks.verify_open_mont_dev(*typed, ok["T"], ws["T"], misses=misses),
           "U": lambda: getattr(E, "verify_%s_mont_dev" % scheme)(*typed, ok["U"], ws["U"]),
           "K": lambda: ks.verify_mont_dev(*typed[:1 + ns], di, typed[-1], ok["K"], ws["K"]),
           "A": lambda: getattr(E, "verify_%s_dev" % scheme)(*aff, ok["A"], ws["A"])}
    fns = {p: fns[p] for p in names}

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
    for p in names:
        assert (v[p] == v["U"]).all(), "%s differs from U at %d items" % (p, int((v[p] != v["U"]).sum()))
    assert int(misses.item()) == nmiss, (int(misses.item()), nmiss)
    out = {"scheme": scheme, "k": k, "n": n, "reps": reps, "miss_share": str(Fraction(share)), "misses": nmiss,
           "fused": fused, "verdicts_equal": True}
    for p in fns:
        out[p if fused or p != "T" else "T2"] = _stats(t[p])
    ks.close()
    return out


def _judge(row):
    """the conditions of one device cell from the fused process's row (with T2 / U2 merged in)"""
    med = lambda p: row[p]["median_ms"]
    spread = round(row["U"]["max_ms"] - row["U"]["min_ms"], 4)
    row["U_spread_ms"] = spread
    row["unkeyed_over_open"] = round(med("U") / med("T"), 3)
    if row["miss_share"] != "1":
        row["cache_pays"] = bool(med("U") - med("T") > spread)
    if "A" in row:
        row["D0_ms"] = round(med("U") - med("A"), 4)
    if "K" in row:
        row["T_minus_K_ms"] = round(med("T") - med("K"), 4)
        row["cost_of_form"] = bool(row["T_minus_K_ms"] <= row["D0_ms"] + spread)
    if "T2" in row:
        row["two_launch_minus_fused_ms"] = round(med("T2") - med("T"), 4)
    return row


def measure_host(scheme, share, k=64, log2_n=20, reps=7):
    import numpy as np

    sys.path.insert(0, ROOT)
    import keyset_bench as KB
    from schnorr_amd import engine as E

    fused = os.environ.get("DSV_OPEN_MONT_FUSED", "1") != "0"
    E.init(0)
    n = 1 << log2_n
    b = _sided_block(E, scheme, k, share, 1357 + k)
    ns = b["nsig"]
    names = ("u", "R", "Rp")[:1 + ns]
    typed = dict(zip(names, b["typed"][:1 + ns]), m=b["typed"][-1])
    typed.setdefault("Rp", None)
    hold = KB._records(scheme, typed, b["typed"][1 + ns:-1], n)
    sigs, pks, msgs, sig_views, key_views = hold
    open_cols = sig_views + key_views + [msgs]
    idx = np.ascontiguousarray(np.tile(b["idx"], n // BLOCK))
    keyed_cols = sig_views + [idx, msgs]
    nmiss = int(b["missed"].sum()) * (n // BLOCK)
    ks = E.KeySet(scheme, *b["reg"])
    got = {}

    def open_call():
        got["open"], got["misses"] = ks.verify_open_mont_cols(open_cols)

    def two_jobs():
        j0, j1 = ks.submit_open_mont_cols(open_cols), ks.submit_open_mont_cols(open_cols)
        got["job0"], got["job1"] = j0.wait(), j1.wait()

    paths = {"open_mont_cols": open_call,
             "mont_cols": lambda: got.__setitem__("unkeyed", E.verify_mont_cols(scheme, open_cols)),
             "open_mont_cols_two_jobs": two_jobs}
    if nmiss == 0:
        paths["keyed_mont_cols"] = lambda: got.__setitem__("keyed", ks.verify_mont_cols(keyed_cols))
    for f in paths.values():
        f()
    t = {p: [] for p in paths}
    trace = os.environ.get("DSV_PIPE_TRACE") is not None  # the library's per-call lines on stderr, labelled by path
    for _ in range(reps):
        for p, f in paths.items():
            if trace:
                sys.stderr.write("[path] %s\n" % p)
                sys.stderr.flush()
            t0 = time.perf_counter()
            f()
            t[p].append((time.perf_counter() - t0) * 1e3)
    assert (got["unkeyed"] == 1).all() and got["misses"] == nmiss, (got["misses"], nmiss)
    for p in got:
        if p != "misses":
            assert (got[p] == got["unkeyed"]).all(), p
    out = {"scheme": scheme, "k": k, "n": n, "reps": reps, "miss_share": str(Fraction(share)), "misses": nmiss,
           "fused": fused, "verdicts_equal": True}
    for p in paths:
        out[p] = _stats(t[p])
    out["open_mont_cols_two_jobs_per_call"] = {x: round(y / 2, 4) for x, y in out["open_mont_cols_two_jobs"].items()}
    un = out["mont_cols"]
    bound = un["median_ms"] + un["max_ms"] - un["min_ms"]
    out["open_not_slower_than_unkeyed"] = bool(out["open_mont_cols"]["median_ms"] <= bound)
    ks.close()
    return out


def soak(total, k=64, log2_n=20):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import keyset_bench as KB
    from schnorr_amd import engine as E

    E.init(0)
    dev = "cuda:0"
    n = 1 << log2_n
    done = calls = falses = differ_dev = differ_host = 0
    schemes = ("single", "double", "vargen")
    while done < total:
        scheme = schemes[calls % 3]
        b = _sided_block(E, scheme, k, Fraction(1, 8), 9000 + calls)
        typed = [c.copy() for c in b["typed"]]
        typed[0][::9, 0] ^= 1  # wrong u on a ninth of the items, under both kinds of key
        ns = b["nsig"]
        times = n // BLOCK
        dcols = [torch.from_numpy(c).to(dev).repeat(times, 1).contiguous() for c in typed]
        ok_t, ok_u = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2))
        with E.KeySet(scheme, *b["reg"]) as ks:
            ks.verify_open_mont_dev(*dcols, ok_t, torch.empty(E.keyed_open_mont_workspace_bytes(scheme, n),
                                                              dtype=torch.uint8, device=dev))
            ws_u = torch.empty(E.mont_workspace_bytes(n), dtype=torch.uint8, device=dev)
            getattr(E, "verify_%s_mont_dev" % scheme)(*dcols, ok_u, ws_u)
            torch.cuda.synchronize()
            names = ("u", "R", "Rp")[:1 + ns]
            tdict = dict(zip(names, typed[:1 + ns]), m=typed[-1])
            tdict.setdefault("Rp", None)
            _, _, msgs, sig_views, key_views = hold = KB._records(scheme, tdict, typed[1 + ns:-1], n)
            host = ks.verify_open_mont_cols(sig_views + key_views + [msgs])[0]
            del hold
        u = ok_u.cpu().numpy()
        differ_dev += int((ok_t.cpu().numpy() != u).sum())
        differ_host += int((host != u).sum())
        falses += int((u == 0).sum())
        done += n
        calls += 1
    return {"verdicts": done, "calls": calls, "false_verdicts": falses, "differ_dev": differ_dev,
            "differ_host": differ_host, "k": k, "n": n}


def _child(args, env_fused, timeout):
    env = dict(os.environ, DSV_OPEN_MONT_FUSED=env_fused)
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True,
                       timeout=timeout, env=env)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit("measurement %s (fused=%s) failed with status %d" % (" ".join(args), env_fused, p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=4, metavar=("SCHEME", "K", "LOG2N", "SHARE"))
    ap.add_argument("--one-host", nargs=2, metavar=("SCHEME", "SHARE"))
    ap.add_argument("--log2-ns", default="14,20")
    ap.add_argument("--ks", default="64,4096")
    ap.add_argument("--shares", default="0,1/64,1/8,1")
    ap.add_argument("--host-shares", default="0,1/8")
    ap.add_argument("--schemes", default="single,double,vargen")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--no-device", action="store_true")
    ap.add_argument("--soak", type=int, default=0)
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    if a.one:
        s, k, l2, share = a.one
        print(json.dumps(measure(s, int(k), int(l2), share, a.reps)), flush=True)
        return
    if a.one_host:
        print(json.dumps(measure_host(a.one_host[0], a.one_host[1])), flush=True)
        return
    doc = {"reps": a.reps, "block": BLOCK, "rows": [], "host_rows": []}

    def save():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)

    if not a.no_device:
        for scheme in a.schemes.split(","):
            for l2 in a.log2_ns.split(","):
                for k in a.ks.split(","):
                    for share in a.shares.split(","):
                        args = ["--one", scheme, k, l2, share, "--reps", str(a.reps)]
                        row = _child(args, "1", a.timeout)
                        two = _child(args, "0", a.timeout)
                        row["T2"], row["U2"] = two["T2"], two["U"]
                        print(json.dumps(_judge(row)), flush=True)
                        doc["rows"].append(row)
                        save()
    if a.host:
        for scheme in a.schemes.split(","):
            for share in a.host_shares.split(","):
                row = _child(["--one-host", scheme, share], "1", a.timeout)
                two = _child(["--one-host", scheme, share], "0", a.timeout)
                row["two_launch"] = {p: two[p] for p in ("open_mont_cols", "mont_cols", "open_mont_cols_two_jobs")}
                print(json.dumps(row), flush=True)
                doc["host_rows"].append(row)
                save()
    if a.soak:
        doc["soak"] = soak(a.soak)
        print(json.dumps(doc["soak"]), flush=True)
        save()


if __name__ == "__main__":
    main()
