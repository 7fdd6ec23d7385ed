"""A few calls of the keyed fast accept on one workload, for a kernel trace (GPU):

    rocprofv3 --kernel-trace -d trace -o tl -- python3 tools/keyed_rlc_case.py single 64 20 valid 3
    python tools/rlc_timeline.py trace/tl_results.db     # the last call, kernel by kernel

SCHEME K LOG2N WORKLOAD CALLS; WORKLOAD: valid | wrong_h8 | wrong_h0 (one wrong item, keyed history set to 8 / 0
before every call)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import numpy as np
    import torch

    from keyset_bench import _signed_batch
    from schnorr_amd import engine as E

    scheme, k, log2_n, workload, calls = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], int(sys.argv[5])
    E.init(0)
    dev = "cuda:0"
    n = 1 << log2_n
    P0, P1, idx, u, R, Rp, m = _signed_batch(E, scheme, k, n, 4321 + k)
    if workload != "valid":
        u[n // 3, 0] ^= 1
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    items = (T(u), T(R)) + ((T(Rp),) if Rp is not None else ()) + (T(idx.view(np.int32)), T(m))
    ks = E.KeySet(scheme, P0, P1)
    ok = torch.empty(n, dtype=torch.uint8, device=dev)
    ws = torch.empty(E.keyed_rlc_workspace_bytes(n, k), dtype=torch.uint8, device=dev)
    acc = torch.zeros(1, dtype=torch.int32, device=dev)
    hist = {"valid": None, "wrong_h8": 8, "wrong_h0": 0}[workload]
    for _ in range(calls):
        if hist is not None:
            E.keyed_rlc_history(0, hist)
        ks.verify_rlc_dev(*items, ok, ws, accepted_out=acc)
        torch.cuda.synchronize()
    print("accepted", int(acc.item()), "true verdicts", int(ok.sum().item()), "of", n)
    ks.close()


if __name__ == "__main__":
    main()
