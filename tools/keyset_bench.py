"""Registered key sets against the unkeyed verify entry points, device-resident inputs (GPU).

    python tools/keyset_bench.py [--out FILE] [--log2-n 20] [--reps 21] [--ks 1,64,4096,16384]
    python tools/keyset_bench.py --one SCHEME K [--reps R]      # one measurement (what the driver runs)

Each (scheme, k) is measured in a process of its own: n items signed under k keys, inputs in HBM, then
dsv_verify_<scheme>_keyed_dev and dsv_verify_<scheme>_dev on the gathered keys alternate on one stream,
each timed with device events after warm-up; the verdict vectors must be equal.  Reported: the median of
the reps per path, the ratio, and the key-set build time per key (dsv_keyset_create, host arrays in,
blocking).  Kernel times: run one measurement under `rocprofv3 --kernel-trace --stats -- python ...`.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=2, metavar=("SCHEME", "K"))
    ap.add_argument("--log2-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--ks", default="1,64,4096,16384")
    ap.add_argument("--schemes", default=",".join(SCHEMES))
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=600)
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
            json.dump({"log2_n": a.log2_n, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
