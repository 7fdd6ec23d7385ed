"""Where a key-set append spends its host time (GPU): the runtime calls an append and a constructor of m keys both
make — stream create / destroy, a 64 KiB hipMalloc / hipFree, a 64-byte pageable copy with its synchronise — each
under a host clock, with a reserved single set of 64 and of 4096 keys (2.4 GB) live in the process, and beside them
the whole dsv_keyset_append of one key to that set (41 in a row) and dsv_keyset_create of one key.  ms: median,
min, max of 41.

    python tools/keyset_append_phases.py [OUT.json]
"""
import ctypes, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from schnorr_amd import engine as E
import torch
E.init(0)
hip = ctypes.CDLL("libamdhip64.so")
def med(f, reps=41, setup=None, done=None):
    ts = []
    for _ in range(reps):
        a = setup() if setup else None
        torch.cuda.synchronize()
        t0 = time.perf_counter(); r = f(a); ts.append((time.perf_counter() - t0) * 1e3)
        if done: done(r)
    ts.sort(); return [round(ts[len(ts) // 2], 4), round(ts[0], 4), round(ts[-1], 4)]
def malloc(_):
    p = ctypes.c_void_p(); assert hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(1 << 16)) == 0; return p
def free(p):
    assert hip.hipFree(p) == 0
def screate(_):
    s = ctypes.c_void_p(); assert hip.hipStreamCreateWithFlags(ctypes.byref(s), 1) == 0; return s
def sdestroy(s):
    assert hip.hipStreamDestroy(s) == 0
host = np.zeros(64, np.uint8)
def copy_sync(sp):
    s, p = sp
    assert hip.hipMemcpyAsync(p, host.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(64), 1, s) == 0
    assert hip.hipStreamSynchronize(s) == 0
    return sp
rng = np.random.default_rng(1)
def keys(n):
    sk = rng.integers(0, 256, size=(n, 32), dtype=np.uint8); sk[:, 31] &= 7
    return E.public_keys(sk)
out = {}
for k in (64, 4096):
    P = keys(k + 64)
    ks = E.KeySet.reserved("single", k + 64, np.ascontiguousarray(P[:k]))
    row = {"hipMalloc_64KiB": med(malloc, done=free), "hipFree": med(free, setup=lambda: malloc(None)),
           "stream_create": med(screate, done=sdestroy), "stream_destroy": med(sdestroy, setup=lambda: screate(None)),
           "copy_64B_and_sync": med(copy_sync, setup=lambda: (screate(None), malloc(None)),
                                    done=lambda sp: (sdestroy(sp[0]), free(sp[1])))}
    it = iter(range(41))
    row["append_m1"] = med(lambda one: ks.append(one), setup=lambda: np.ascontiguousarray(P[k + next(it):][:1]))
    one = np.ascontiguousarray(P[:1])
    row["create_m1"] = med(lambda _: E.KeySet("single", one), done=lambda s: s.close())
    out["live_k_%d" % k] = row
    print(k, json.dumps(row), flush=True)
    ks.close()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
