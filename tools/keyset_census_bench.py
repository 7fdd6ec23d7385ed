"""The key census (dsv_keyset_census_dev) against the lookup it repeats, the open-set verify call it stands next to,
and the host alternative it replaces; device-resident inputs (GPU).

    python tools/keyset_census_bench.py [--out profiles/keyset/keyset_census_bench.json] [--log2-n 20] [--reps 21]
                                        [--ks 64,16384]
    python tools/keyset_census_bench.py --one K SHARE SPREAD [--log2-n 20] [--reps R]   # one cell (what the driver runs)

Each cell is measured in a process of its own under a time limit, profiler off, a failed cell ends the run: n
all-valid single-scheme items in HBM over a set of K registered keys; round(SHARE * n) of them at random positions
are signed under valid keys that are NOT registered, and SPREAD says how many such keys there are — "1", "1024" or
"distinct" (one key per missed item); the rest are uniform over the K registered keys, or, for SPREAD "hot" (share 0
only), all under ONE registered key.  On identical items, alternating on one stream, each call timed with device
events after warm-up:
  C   KeySet.census_dev with key_idx_out and hits
  L   KeySet.lookup_dev on the same key column (dsv_keyset_lookup_dev)
  T   KeySet.verify_open_dev on the same items
  H   the host alternative, wall clock, 3 runs: the index column and the key column copied back, numpy counting the
      hits (bincount) and the distinct missed keys (unique over the missed rows)
C's outputs must be the numpy result's.  Reported per cell: medians with min and max, census_over_lookup,
census_over_open, host_over_census.  Conditions, evaluated over the cells (none is a test):
  (a) census_within_2x_lookup     every share-0 cell: C <= 2 L
  (b) hot_over_uniform            C of "every item under one registered key" / C of "uniform over the K keys", and
      one_over_1024_missed_keys   C of "all misses under 1 key" / C of "misses under 1024 keys", per share: far above
                                  1 = contention
  (c) census_over_open            what a caller pays for the policy's input, per cell
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
CELLS = [("0", "uniform"), ("0", "hot"), ("1/8", "1"), ("1/8", "1024"), ("1/8", "distinct"), ("1", "1"), ("1", "1024"),
         ("1", "distinct")]


def _stats(v):
    v = sorted(v)
    return {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}


def measure(k, share, spread, log2_n, reps, warmup=3):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from keyset_bench import _scalars
    from schnorr_amd import engine as E

    E.init(0)
    dev = "cuda:0"
    n = 1 << log2_n
    nmiss = int(round(Fraction(share) * n))
    rng = np.random.default_rng(2468 + k)
    strangers = {"uniform": 0, "hot": 0, "1": 1, "1024": 1024, "distinct": nmiss}[spread] if nmiss else 0
    sk = _scalars(rng, k + strangers, 0x07)
    K0 = E.public_keys(sk)
    missed = np.zeros(n, bool)
    missed[rng.permutation(n)[:nmiss]] = True
    idx = np.full(n, 7 % k) if spread == "hot" else rng.integers(0, k, size=n)
    if nmiss:
        idx[missed] = k + (np.arange(nmiss) if spread == "distinct" else rng.integers(0, strangers, size=nmiss))
    m, r = _scalars(rng, n, 0x3F), _scalars(rng, n, 0x07)
    u, R = E.sign_single(sk[idx], m, r)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    PK = K0[idx]
    d_all = [T(c) for c in (u, R, PK, m)]
    ks = E.KeySet("single", np.ascontiguousarray(K0[:k]))
    assert (ks.key_ok() == 1).all()
    new = lambda count, dtype=torch.int32: torch.zeros(count, dtype=dtype, device=dev)
    c_idx, l_idx, hits, rep, count, totals = new(n), new(n), new(k), new(n), new(n), new(4)
    c_ws = new(E.keyset_census_workspace_bytes(n), torch.uint8)
    ok, t_miss = new(n, torch.uint8), new(1)
    t_ws = new(E.keyed_open_workspace_bytes(n), torch.uint8)
    fns = {"C": lambda: ks.census_dev(d_all[2], c_idx, hits, rep, count, totals, c_ws),
           "L": lambda: ks.lookup_dev(d_all[2], l_idx),
           "T": lambda: ks.verify_open_dev(*d_all, ok, t_ws, misses=t_miss)}

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

    def host():  # what a caller did without the census: copy back, count with numpy
        t0 = time.perf_counter()
        i = l_idx.cpu().numpy().view(np.uint32)
        keys = d_all[2].cpu().numpy()
        at = np.flatnonzero(i == E.KEY_NONE)
        h = np.bincount(i[i != E.KEY_NONE], minlength=k)
        if len(at):
            _, first, c = np.unique(keys[at].view("V64").ravel(), return_index=True, return_counts=True)
        else:
            first, c = np.zeros(0, np.int64), np.zeros(0, np.int64)
        return (time.perf_counter() - t0) * 1e3, h, {(int(at[f]), int(x)) for f, x in zip(first, c)}

    host_ms = []
    for _ in range(3):
        ms, h, report = host()
        host_ms.append(ms)
    # the census's outputs are the numpy result's
    hits.zero_()
    fns["C"]()
    torch.cuda.synchronize()
    tot = totals.cpu().numpy().view(np.uint32)
    d = int(tot[0])
    got = set(zip(rep[:d].cpu().numpy().view(np.uint32).tolist(), count[:d].cpu().numpy().view(np.uint32).tolist()))
    assert got == report and tot.tolist() == [len(report), nmiss, 0, 0], (d, len(report), tot)
    assert (hits.cpu().numpy() == h).all() and torch.equal(c_idx, l_idx)
    assert (ok.cpu().numpy() == 1).all() and int(t_miss.item()) == nmiss

    out = {"k": k, "n": n, "reps": reps, "miss_share": str(Fraction(share)), "spread": spread, "misses": nmiss,
           "distinct_missed_keys": len(report), "lds_keys": E.census_lds_keys(), "outputs_equal_numpy": True}
    for p in fns:
        out[p] = _stats(t[p])
    out["H"] = _stats(host_ms)
    med = lambda p: out[p]["median_ms"]
    out["census_over_lookup"] = round(med("C") / med("L"), 3)
    out["census_over_open"] = round(med("C") / med("T"), 4)
    out["host_over_census"] = round(med("H") / med("C"), 1)
    ks.close()
    return out


def conditions(rows):
    cell = {(r["k"], r["miss_share"], r["spread"]): r for r in rows}
    c = lambda key: cell[key]["C"]["median_ms"]
    out = {"census_within_2x_lookup": {}, "hot_over_uniform": {}, "one_over_1024_missed_keys": {}, "census_over_open": {}}
    for (k, share, spread), r in cell.items():
        name = "k=%d share=%s %s" % (k, share, spread)
        out["census_over_open"][name] = r["census_over_open"]
        if share == "0":
            out["census_within_2x_lookup"][name] = {"holds": bool(r["census_over_lookup"] <= 2.0),
                                                    "census_over_lookup": r["census_over_lookup"]}
        if spread == "hot" and (k, "0", "uniform") in cell:
            out["hot_over_uniform"]["k=%d" % k] = round(c((k, share, spread)) / c((k, "0", "uniform")), 3)
        if spread == "1" and (k, share, "1024") in cell:
            out["one_over_1024_missed_keys"]["k=%d share=%s" % (k, share)] = round(
                c((k, share, "1")) / c((k, share, "1024")), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=3, metavar=("K", "SHARE", "SPREAD"))
    ap.add_argument("--log2-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--ks", default="64,16384")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyset", "keyset_census_bench.json"))
    ap.add_argument("--timeout", type=int, default=300)
    a = ap.parse_args()
    if a.one:
        print(json.dumps(measure(int(a.one[0]), a.one[1], a.one[2], a.log2_n, a.reps)), flush=True)
        return
    rows = []
    for k in (int(x) for x in a.ks.split(",")):
        for share, spread in CELLS:
            cmd = [sys.executable, os.path.abspath(__file__), "--one", str(k), share, spread, "--log2-n",
                   str(a.log2_n), "--reps", str(a.reps)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
            if p.returncode != 0:
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit("measurement k=%d s=%s %s failed with status %d" % (k, share, spread, p.returncode))
            row = json.loads(p.stdout.strip().splitlines()[-1])
            print(json.dumps(row), flush=True)
            rows.append(row)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump({"log2_n": a.log2_n, "reps": a.reps, "rows": rows, "conditions": conditions(rows)}, f,
                          indent=1)
    print(json.dumps(conditions(rows)), flush=True)


if __name__ == "__main__":
    main()
