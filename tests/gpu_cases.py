"""Builders and runners the unkeyed GPU suites share (tests/test_gpu_r02.py ... r06.py, test_gpu_rlc*.py): a device
copy of one array, the mixed single / double batch, and the fast accept's signed batches, oracle call and runner.
The child process of tests/test_gpu_r06.py imports this module too."""
import numpy as np
import torch

import harness as H
import oracle_lib as O
import pymodel as M

DEV = "cuda:0"
COLS = {"single": ("u", "R", "PK", "m"), "double": ("u", "R", "Rp", "PK", "PKp", "m"),
        "vargen": ("u", "R", "PK", "Gen", "m")}


def _dev_col(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _mixed_arrays(n, seed):
    rng = np.random.default_rng(seed)
    kinds = rng.integers(0, 2, size=n, dtype=np.uint8)
    si, di = np.nonzero(kinds == 0)[0], np.nonzero(kinds == 1)[0]
    ds = O.keygen_sign_single(len(si), seed, nthreads=8)
    dd = O.keygen_sign_double(len(di), seed + 1, nthreads=8)
    H.tamper(ds, period=5)
    H.tamper(dd, period=7)
    cols = {k: np.zeros((n, w), np.uint8) for k, w in (("u", 32), ("R", 64), ("Rp", 64), ("PK", 64),
                                                       ("PKp", 64), ("m", 32))}
    for k in ("u", "R", "PK", "m"):
        cols[k][si] = ds[k]
    for k in cols:
        cols[k][di] = dd[k]
    want = np.zeros(n, np.uint8)
    want[si] = O.verify_single(ds["u"], ds["R"], ds["PK"], ds["m"], nthreads=8)
    want[di] = O.verify_double(dd["u"], dd["R"], dd["Rp"], dd["PK"], dd["PKp"], dd["m"], nthreads=8)
    return kinds, cols, want, len(di)


# ---- the batch fast accept -----------------------------------------------------------------------------------
def _scheme_of(a):
    return "double" if "Rp" in a else ("vargen" if "Gen" in a else "single")


def _run(engine, a, scheme=None, window_bits=0, **kw):
    """(accepted, verdicts) of verify_<scheme>_rlc_dev on the batch's columns, ok poisoned first; the scheme is
    read off the columns unless given; kw (accepted_out) goes to the call as it is"""
    scheme = scheme or _scheme_of(a)
    n = len(a["u"])
    t = [torch.from_numpy(np.ascontiguousarray(a[k])).to(DEV) for k in COLS[scheme]]
    ok = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    ws = torch.empty(engine.rlc_workspace_bytes(n, window_bits), dtype=torch.uint8, device=DEV)
    accepted = getattr(engine, "verify_%s_rlc_dev" % scheme)(*t, ok, ws, window_bits=window_bits, **kw)
    torch.cuda.synchronize()
    return accepted, ok.cpu().numpy()


def _oracle(a, scheme=None):
    scheme = scheme or _scheme_of(a)
    return getattr(O, "verify_" + scheme)(*[a[k] for k in COLS[scheme]], nthreads=8)


def _signed(n, seed, scheme="single"):
    d = getattr(O, "keygen_sign_" + scheme)(n, seed, nthreads=8)
    return {k: d[k] for k in COLS[scheme]}


def _torsion_rows(t8, rnd, count, cancel):
    """signatures whose key and nonce point carry order-8 components; `cancel`: c*k1 == k2 (mod 8),
    i.e. VALID under the reference's cofactorless equation"""
    rows = {"u": [], "R": [], "PK": [], "m": []}
    while len(rows["u"]) < count:
        sk, m, rr = rnd.randrange(1, M.R_ORDER), rnd.randrange(M.Q), rnd.randrange(1, M.R_ORDER)
        k1, k2 = rnd.randrange(1, 8), rnd.randrange(8)
        pk = M.padd(M.pmul(M.GEN, sk), M.pmul(t8, k1))
        R = M.padd(M.pmul(M.GEN, rr), M.pmul(t8, k2))
        c = M.challenge(R, m)
        if ((c * k1 - k2) % 8 == 0) != cancel:
            continue
        rows["u"].append(np.frombuffer(M.le32((rr - c * sk) % M.R_ORDER), np.uint8))
        rows["R"].append(np.frombuffer(M.point_bytes(R), np.uint8))
        rows["PK"].append(np.frombuffer(M.point_bytes(pk), np.uint8))
        rows["m"].append(np.frombuffer(M.le32(m), np.uint8))
    return {k: np.stack(v) for k, v in rows.items()}
