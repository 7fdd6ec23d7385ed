"""GPU tests of what round 4 added.  Parity is always against the CPU oracle (oracle/).

* dsv_verify_{single,double,vargen}_mont[_multi|_dev|_cols]: the reference's IN-MEMORY representation
  (four u64 Montgomery limbs per element, R = 2^256: /root/reference/Cargo.toml:25-26,
  src/signatures.rs:58-61, src/keys/public.rs:59) — dense arrays, device pointers, and the typed
  objects read in place as strided columns.
"""
import os

import numpy as np
import pytest

import mont_cases as C
import pymodel as M
import oracle_lib as O
from gpu_cases import _dev_col

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = {"single": 31, "double": 32, "vargen": 33}


@pytest.mark.parametrize("scheme", ["single", "double", "vargen"])
def test_montgomery_limb_entry_points_match_the_oracle(engine, scheme):
    """Tampered items, random z per point, z = 0, coordinate / message limbs >= q, u limbs >= r —
    through the host entry point, the sharded one, the device-pointer one and the strided columns of
    record arrays laid out like the Rust structs."""
    import torch
    n = 300 + 13
    cols, want = C.mont_case(scheme, n, SEEDS[scheme])
    assert 0 < want.sum() < n
    host = getattr(engine, "verify_%s_mont" % scheme)
    assert np.array_equal(host(*cols), want)
    # the typed objects where they lie: Signature { u, R: JubJubExtended(160 B) }, PublicKey(160 B) ...
    sigs, pks, msgs, views = C.as_records(scheme, cols)
    assert np.array_equal(engine.verify_mont_cols(scheme, views), want)
    os.environ["DSV_MULTI_SHARDS"] = "3"          # the sharding arithmetic (offset * stride) on one GPU
    try:
        reps = 12                                  # below nd * 1024 items the multi form takes one device
        tile = lambda a: np.tile(a, (reps, 1))
        assert np.array_equal(host(*[tile(c) for c in cols], multi=True), np.tile(want, reps))
        big = C.as_records(scheme, [tile(c) for c in cols])[3]
        assert np.array_equal(engine.verify_mont_cols(scheme, big), np.tile(want, reps))
    finally:
        del os.environ["DSV_MULTI_SHARDS"]
    ok = torch.full((n,), 9, dtype=torch.uint8, device="cuda:0")
    ws = torch.full((engine.mont_workspace_bytes(n),), 0xFF, dtype=torch.uint8, device="cuda:0")
    getattr(engine, "verify_%s_mont_dev" % scheme)(*[_dev_col(c) for c in cols], ok, ws)
    torch.cuda.synchronize()
    assert np.array_equal(ok.cpu().numpy(), want)


def test_montgomery_limbs_equal_the_projective_entry_point_on_to_bytes(engine):
    """`_mont` on the limbs == `_ext` on the to_bytes() of the same values (the oracle does the
    conversion), on a batch large enough for the chunked pipeline, the multi-threaded strided gather
    and the one-inversion-per-16-items normalisation."""
    scheme, base = "single", 509
    cols, want = C.mont_case(scheme, base, 77, period=5)
    n = (1 << 16) + 4099
    reps = -(-n // base)
    tile = lambda a: np.ascontiguousarray(np.tile(a, (reps, 1))[:n])
    tcols = [tile(c) for c in cols]
    twant = np.tile(want, reps)[:n]
    views = C.as_records(scheme, tcols)[3]
    got = engine.verify_mont_cols(scheme, views)
    assert np.array_equal(got, twant)
    assert np.array_equal(engine.verify_single_mont(*tcols), twant)
    # canonical bytes of the same values through the r03 projective path
    canon = [O.from_mont(tcols[0], fr=True)[0]] + [O.from_mont(c)[0] for c in tcols[1:]]
    bad = (got != engine.verify_single_ext(*canon))
    # the two paths may only differ where limbs were not below the modulus (no canonical form)
    planted = np.flatnonzero(bad) % base
    assert len(set(planted.tolist())) <= 4 and not twant[bad].any()


@pytest.mark.parametrize("scheme", ["double", "vargen"])
def test_montgomery_record_columns_across_several_chunks(engine, scheme):
    """The strided gather out of record arrays for the six- and five-column schemes on a batch that
    takes several pipeline chunks and sub-batches (2^16 + 2^15 + a ragged tail), with one and with four
    copy threads: every chunk's whole-chunk normalisation, both compute lanes, per-slot scratch."""
    base = 211
    cols, want = C.mont_case(scheme, base, SEEDS[scheme] + 100, period=4)
    n = (1 << 16) + (1 << 15) + 77
    reps = -(-n // base)
    tcols = [np.ascontiguousarray(np.tile(c, (reps, 1))[:n]) for c in cols]
    twant = np.tile(want, reps)[:n]
    views = C.as_records(scheme, tcols)[3]
    try:
        for threads in (1, 4):
            assert engine.set_host_threads(threads) == threads
            assert np.array_equal(engine.verify_mont_cols(scheme, views), twant), threads
    finally:
        engine.set_host_threads(0)
    assert 0 < twant.sum() < n


def test_montgomery_column_arguments_are_validated(engine):
    cols, _ = C.mont_case("single", 8, 5, plant=False)
    with pytest.raises(ValueError):
        engine.verify_mont_cols("single", cols[:3])
    with pytest.raises(ValueError):
        engine.verify_mont_cols("single", [cols[0], cols[1][:, :64], cols[2], cols[3]])
    from schnorr_amd import _lib
    import ctypes
    arr = (_lib.Column * 4)()
    for k, c in enumerate(cols):
        arr[k].base, arr[k].stride = c.ctypes.data, c.strides[0]
    arr[1].stride = 64                            # a 96-byte field cannot repeat every 64 bytes
    ok = np.zeros(8, np.uint8)
    rc = _lib.load().dsv_verify_single_mont_cols(arr, ctypes.c_size_t(8), ctypes.c_void_p(ok.ctypes.data))
    assert rc == -2 and b"stride" in _lib.load().dsv_last_error()
    assert _lib.load().dsv_verify_single_mont_cols(arr, ctypes.c_size_t(0), None) == 0   # empty batch


def test_vargen_kernel_on_its_fallback_row_in_a_test_build(engine):
    """lattice3.h falls back to the row (u, c, 1) — the reference equation as a 63-window chain with a
    252-bit x = u — when no reduced row has an odd z below 2^251; no hash output steers a challenge
    there, so the branch is exercised in a TEST BUILD whose reduction does no batch at all
    (schnorr_amd/libdsv_lat0.so: -DDSV_LAT_MAX_BATCHES=0 on k_vargen.hip only): every item
    takes the fallback, and the var-generator tampering / torsion / projective / wire tests must still
    equal the oracle."""
    import subprocess
    import sys
    from schnorr_amd import build as B
    lib = B.variant_path("lat0")
    assert os.path.exists(lib), "run __graft_entry__.build() first: it makes the lat0 test build"
    # the fallback really is what this build computes: (x, y, z) = (u, c, 1) for arbitrary inputs
    probe = ("import numpy as np; from schnorr_amd import engine as E; E.init(0); "
             "u = np.arange(64, dtype=np.uint8).reshape(2, 32); u[:, 31] &= 7; c = u[::-1].copy(); c[:, 31] &= 3; "
             "le = lambda r: int.from_bytes(bytes(r), 'little'); "
             "assert E.debug_lattice3(u, c) == [(le(u[i]), le(c[i]), 1) for i in range(2)]; print('fallback ok')")
    env = dict(os.environ, DSV_LIB_PATH=lib)
    r = subprocess.run([sys.executable, "-c", probe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fallback ok" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])
    expr = "vargen and not lattice and not config_size and not input_stream and not fallback_row"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_parity.py"),
                        os.path.join(ROOT, "tests", "test_gpu_r03.py"), os.path.join(ROOT, "tests", "test_gpu_r04.py"),
                        "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-k", expr],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-500:]


def test_bench_under_the_drivers_launcher(engine):
    """The driver starts N > 1 as `python -m torch.distributed.run --nnodes=1 --nproc-per-node N
    --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...`: rehearsed with two ranks on this
    one GPU over gloo (DSV_BENCH_DEVICE / DSV_BENCH_BACKEND); the line must come from rank 0 alone, be
    the last line of stdout, name the launcher and carry the per-rank fields."""
    import json
    import socket
    import subprocess
    import sys
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    drop = ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update({"DSV_BENCH_DEVICE": "0", "DSV_BENCH_BACKEND": "gloo"})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "2", "--warmup", "1", "--log2-batch", "14", "--no-cpu-baseline", "--full"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.strip().splitlines() if l.strip()]
    json_lines = [l for l in lines if l.startswith("{")]
    assert len(json_lines) == 1 and lines[-1] == json_lines[0], lines[-3:]
    line = json.loads(json_lines[0])
    assert line["launcher"] == "torch.distributed.run" and line["n_gpus"] == 2 and line["backend"] == "gloo"
    assert line["steps"] == 2 and line["warmup"] == 1 and line["value"] > 0
    assert len(line["ranks"]["ms_per_step"]["all"]) == 2 and line["mixed"]["n_gpus"] == 2
    assert abs(line["value"] - 2 * (1 << 14) * 2 / (line["ms_per_step"] * 2 / 1e3)) < 1e-6 * line["value"]


def test_inversion_edge_values_through_to_hash_inputs(engine):
    """k_normalize_uvz inverts by the extended Euclidean algorithm with float-guided quotients
    (inv29.h) and falls back to Fermat for z = 0, for quotients beyond 31 bits (z = 1, 2, small z) and at
    the iteration cap: `dsv_to_hash_inputs` against Python integers on z values at both ends of the
    range, powers of two and their neighbours, values whose Euclidean quotients are huge or all 1
    (Fibonacci-like), and random ones — alone (one inversion per point) and in a batch large enough
    for sixteen points to share one inversion (the product of their z's is what gets inverted)."""
    import random
    rnd = random.Random(2718)
    q = M.Q
    fib = [1, 2]
    while fib[-1] < q:
        fib.append(fib[-1] + fib[-2])
    zs = [1, 2, 3, 5, 255, 256, (1 << 31) - 1, 1 << 31, (1 << 32) + 1, q - 1, q - 2, (q - 1) // 2, (q + 1) // 2,
          q // 3, q // 3 + 1, (1 << 128) - 1, 1 << 128, (1 << 254) + 12345, fib[-2], fib[-3], q - fib[-4],
          pow(2, -1, q), pow(3, -1, q), pow(7, 200, q)]
    zs += [1 << k for k in range(1, 255, 17)] + [(1 << k) - 1 for k in range(2, 255, 19)]
    zs += [q // d for d in (5, 17, 257, 65537, (1 << 31) - 1, (1 << 40) + 3)]
    zs += [rnd.randrange(1, q) for _ in range(400)] + [rnd.randrange(1, 1 << rnd.randrange(1, 255)) for _ in range(200)]
    u0, v0 = M.GEN
    def rows(zlist):
        a = np.zeros((len(zlist), 96), np.uint8)
        for i, z in enumerate(zlist):
            uu, vv = (u0 + i) % q, (v0 * (i + 1)) % q           # any field elements will do here
            a[i] = np.frombuffer(M.le32(uu * z % q) + M.le32(vv * z % q) + M.le32(z), np.uint8)
        return a
    def check(zlist):
        out, ok = engine.to_hash_inputs(rows(zlist))
        assert ok.all()
        for i in range(len(zlist)):
            assert M.from_le(out[i, :32]) == (u0 + i) % q and M.from_le(out[i, 32:]) == (v0 * (i + 1)) % q, (i, zlist[i])
    check(zs)                                    # n < 2^15: one inversion per point
    big = (zs * (-(-((1 << 15) + 100) // len(zs))))[:(1 << 15) + 100]
    check(big)                                   # eight points per inversion
    zero = rows([0, 5, 0, 7])
    out, ok = engine.to_hash_inputs(zero)
    assert ok.tolist() == [0, 1, 0, 1]


def test_mixed_batch_at_the_full_configs4_size_on_one_gpu(engine):
    """BASELINE.json configs[4] is 2^23 mixed single + double signatures over 8 GPUs; no 8-GPU node has
    been available, so here the WHOLE 2^23-item batch (2^22 single on even, 2^22 double on odd
    positions, one structure of arrays, 2.7 GB of inputs) goes through dsv_verify_mixed_dev on one
    GPU — the device-side split, gathers, both kernels' sub-batch loops and the scatter at the stated
    size — AND through the rank-sharded verifier as eight consecutive 2^20-item shards of the same
    global batch (what ranks 0..7 would each hold), whose verdicts must tile the unsharded ones.
    Pattern-checked everywhere, the oracle on a random sample."""
    import torch
    from schnorr_amd import workload as W
    from schnorr_amd.distributed import MixedShardedVerifier
    n = 1 << 23
    mb = W.gen_mixed(n, seed=2321)
    ok = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    ws = torch.empty(engine.mixed_workspace_bytes(n), dtype=torch.uint8, device="cuda:0")
    engine.verify_mixed_dev(mb["kinds"], mb["u"], mb["R"], mb["Rp"], mb["PK"], mb["PKp"], mb["m"], mb["n_double"], ok, ws)
    torch.cuda.synchronize()
    assert int((ok != mb["expected"]).sum().item()) == 0
    assert 0.9 * n < int(ok.sum().item()) < n
    del ws
    # the eight shards a node's ranks would hold (first_item = rank * 2^20 of the same streams)
    shard = 1 << 20
    ver = MixedShardedVerifier(shard, shard // 2, 1, 0, "cuda:0", collective=False)
    gk = (torch.arange(shard, device="cuda:0") & 1).to(torch.uint8)
    for rank in (0, 3, 7):
        part = W.gen_mixed(shard, seed=2321, first_item=rank * shard)
        got = ver(part, gk)
        torch.cuda.synchronize()
        assert torch.equal(got, ok[rank * shard:(rank + 1) * shard]), rank
    # oracle on a random sample of the big batch
    rng = np.random.default_rng(5)
    idx = np.sort(rng.choice(n, 1024, replace=False))
    sel = torch.from_numpy(idx).to("cuda:0")
    cols = {k: mb[k][sel].cpu().numpy() for k in ("u", "R", "Rp", "PK", "PKp", "m")}
    kinds = idx & 1
    want = np.zeros(len(idx), np.uint8)
    s_, d_ = kinds == 0, kinds == 1
    want[s_] = O.verify_single(cols["u"][s_], cols["R"][s_], cols["PK"][s_], cols["m"][s_], nthreads=8)
    want[d_] = O.verify_double(*(cols[k][d_] for k in ("u", "R", "Rp", "PK", "PKp", "m")), nthreads=8)
    assert np.array_equal(want, ok[sel].cpu().numpy())
