"""The keyed wire form on the GPU (dsv_verify_*_keyed_wire*, KeySet.verify_wire / verify_wire_dev): serialized
signatures against a registered key set.  Whole-vector equality everywhere: with the oracle's wire verdicts on
the gathered key records, with the adversarial wire base sets registered by unique key record, with the
composed path (decompress, keyed verify, AND of the decode flags), with the unkeyed wire entry points at 2^20
items; index checks, the _dev contract, the host form at the host pipeline's edges, lifetime and shutdown."""
import ctypes
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import dispatch_edges as D
import edge_sets as ES
import pymodel as M
import keyed_cases as KC
from keyed_cases import _diff, _enc, _key_records, _non_squares, _oracle_wire, _poison, _sig, _to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMES = ("single", "double", "vargen")
NS = (1, 63, 64, 65, 4099, (1 << 16) + 3)
SIG_BYTES = {"single": 64, "double": 96, "vargen": 64}
Q = M.Q


_WIRE = {}


def _wire_batch(engine, scheme, k, n):
    """keyed_cases._batch serialized: sig, idx, m, the key records and the oracle's wire verdicts"""
    key = (scheme, k, n)
    if key not in _WIRE:
        b = KC._batch(engine, scheme, k, n)
        sig = _sig(b["u"], b["R"], b["Rp"])
        rec = _key_records(b["P0"], b["P1"])
        want = _oracle_wire(scheme, sig, rec[b["idx"]], b["m"])
        if len(_WIRE) > 4:
            _WIRE.pop(next(iter(_WIRE)))
        _WIRE[key] = {"sig": sig, "idx": b["idx"].copy(), "m": b["m"], "rec": rec, "want": want, "P0": b["P0"],
                      "P1": b["P1"]}
    return _WIRE[key]


def _run_wire_dev(engine, ks, dsig, didx, dm, n, stream=None):
    ok = _poison(n)
    ws = torch.empty(max(engine.keyed_wire_workspace_bytes(ks.scheme, n), 1), dtype=torch.uint8, device=DEV)
    ks.verify_wire_dev(dsig[:n], didx[:n], dm[:n], ok, ws, stream=stream)
    torch.cuda.synchronize()
    return ok.cpu().numpy()


def _wire_dev(engine, ks, sig, idx, m):
    return _run_wire_dev(engine, ks, _to_dev(sig), _to_dev(idx), _to_dev(m), len(m))


# ---- oracle parity ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 37, 1000))
@pytest.mark.parametrize("scheme", SCHEMES)
def test_oracle_parity(engine, scheme, k):
    b = _wire_batch(engine, scheme, k, NS[-1])
    want = b["want"]
    assert 0 < want.sum() < len(want)
    with engine.KeySet.from_wire(scheme, b["rec"]) as ks:
        assert ks.k == k and (ks.key_ok() == 1).all()
        dsig, didx, dm = _to_dev(b["sig"]), _to_dev(b["idx"]), _to_dev(b["m"])
        for n in NS:
            got = _run_wire_dev(engine, ks, dsig, didx, dm, n)
            assert (got == want[:n]).all(), (scheme, k, n, _diff(got, want[:n]))
            if n <= 4099:
                host = ks.verify_wire(b["sig"][:n], b["idx"][:n], b["m"][:n])
                assert (host == want[:n]).all(), (scheme, k, n, _diff(host, want[:n]))


# ---- adversarial wire base sets, registered by unique key record ------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_adversarial_wire_set(engine, scheme):
    (sig, pk, m), want = ES.base(scheme, "wire", "mixed")
    uniq, inv = np.unique(pk, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1).astype(np.uint32)
    uniq = np.ascontiguousarray(uniq)
    assert len(want) == 2273 and 0 < want.sum() < len(want)
    # the oracle alone fixes every expected verdict, undecodable keys included
    assert (_oracle_wire(scheme, sig, uniq[inv], m) == want).all()
    with engine.KeySet.from_wire(scheme, uniq) as ks:
        assert ks.k == len(uniq)
        got = _wire_dev(engine, ks, sig, inv, m)
        assert (got == want).all(), _diff(got, want)
        host = ks.verify_wire(sig, inv, m)
        assert (host == want).all(), _diff(host, want)


# ---- the composed path: decompress, keyed verify, AND of the decode flags ---------------------------------
def _plant_undecodable(scheme, sig, want_rows):
    """rows of honest items -> sig with undecodable and special nonce encodings planted; returns the planted
    (row, what) list.  Column 32:64 is R, 64:96 (double) R'."""
    sig = sig.copy()
    ns = _non_squares(4)
    vq = _enc(Q, 0)
    rows = iter(want_rows)
    planted = []
    for col, name in ((32, "R"),) + (((64, "Rp"),) if scheme == "double" else ()):
        for enc, what in ((vq, "v=q"), (ns[0], "nonsquare"), (ns[1], "nonsquare"), (_enc((1 << 255) - 1, 1), "ones")):
            i = next(rows)
            sig[i, col:col + 32] = enc
            planted.append((i, name + ":" + what, False))
        # the sign bit set on u = 0 (v = 1: the identity, v = q - 1: the point of order 2): decodable
        for enc in (_enc(1, 1), _enc(Q - 1, 1), _enc(1, 0)):
            i = next(rows)
            sig[i, col:col + 32] = enc
            planted.append((i, name + ":u=0", True))
    if scheme == "double":  # both points of one item undecodable
        i = next(rows)
        sig[i, 32:64], sig[i, 64:96] = vq, ns[2]
        planted.append((i, "R,Rp", False))
    return sig, planted


@pytest.mark.parametrize("k", (1, 37))
@pytest.mark.parametrize("scheme", SCHEMES)
def test_equals_composed_path(engine, scheme, k):
    b = _wire_batch(engine, scheme, k, NS[-1])
    honest = np.flatnonzero(b["want"] == 1)
    # spread over the batch, some of them lane neighbours
    rows = np.concatenate([honest[:8], honest[len(honest) // 2:len(honest) // 2 + 8], honest[-8:]])
    sig, planted = _plant_undecodable(scheme, b["sig"], rows.tolist())
    n = len(sig)
    npts = 2 if scheme == "double" else 1
    cols, flags = [], np.ones(n, np.uint8)
    for p in range(npts):
        uv, ok = engine.decompress_points(np.ascontiguousarray(sig[:, 32 + 32 * p:64 + 32 * p]))
        cols.append(uv)
        flags &= ok
    for i, what, decodable in planted:
        assert flags[i] == (1 if decodable else 0), (i, what)
    assert (flags == 0).sum() == sum(1 for p in planted if not p[2])
    u = np.ascontiguousarray(sig[:, :32])
    with KC._keyset(engine, scheme, b) as ks:
        composed = KC._run_dev(engine, ks, KC._dev([u] + cols + [b["idx"], b["m"]]), n) & flags
        dsig, didx, dm = _to_dev(sig), _to_dev(b["idx"]), _to_dev(b["m"])
        for nn in NS:
            got = _run_wire_dev(engine, ks, dsig, didx, dm, nn)
            assert (got == composed[:nn]).all(), (scheme, k, nn, _diff(got, composed[:nn]))
        host = ks.verify_wire(sig, b["idx"], b["m"])
        assert (host == composed).all(), _diff(host, composed)
    want = _oracle_wire(scheme, sig, b["rec"][b["idx"]], b["m"])
    assert (composed == want).all(), _diff(composed, want)
    for i, what, decodable in planted:
        if not decodable:
            assert composed[i] == 0, (i, what)


# ---- 2^20 items against the unkeyed wire entry points -----------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_two_pow_20_matches_unkeyed_wire(engine, scheme):
    n, k = 1 << 20, 64
    sk, gen, P0, P1 = KC._keys(engine, scheme, k, 4242)
    rng = np.random.default_rng(99)
    idx = rng.integers(0, k, size=n).astype(np.uint32)
    m = KC._scalars(rng, n, 0x3F)
    r = KC._scalars(rng, n, 0x07)
    Rp = None
    if scheme == "single":
        u, R = engine.sign_single(sk[idx], m, r)
    elif scheme == "double":
        u, R, Rp = engine.sign_double(sk[idx], m, r)
    else:
        u, R = engine.sign_vargen(sk[idx], gen[idx], m, r)
    # every 16th item: another key's index (a signature checked against the wrong key), every 16th + 5: u + 1
    idx[::16] = (idx[::16] + 1) % k
    u[5::16, 0] ^= 1
    sig = _sig(u, R, Rp)
    rec = _key_records(P0, P1)
    dsig, didx, dm = _to_dev(sig), _to_dev(idx), _to_dev(m)
    with engine.KeySet(scheme, P0, P1) as ks:
        got = _run_wire_dev(engine, ks, dsig, didx, dm, n)
    dpk = _to_dev(rec[idx])
    ok = _poison(n)
    ws = torch.empty(engine.wire_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    getattr(engine, "verify_%s_wire_dev" % scheme)(dsig, dpk, dm, ok, ws)
    torch.cuda.synchronize()
    ref = ok.cpu().numpy()
    assert (got == ref).all(), _diff(got, ref)
    assert 0.8 < got.mean() < 0.9
    sample = np.sort(rng.choice(n, 4096, replace=False))
    want = _oracle_wire(scheme, sig[sample], rec[idx[sample]], m[sample])
    assert (got[sample] == want).all(), _diff(got[sample], want)


# ---- indices and invalid keys -----------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_index_checks(engine, scheme):
    b = _wire_batch(engine, scheme, 37, 4099)
    idx = b["idx"].copy()
    honest = np.flatnonzero(b["want"] == 1)
    bad = honest[:4]
    idx[bad[0]], idx[bad[1]], idx[bad[2]] = 37, 1 << 31, (1 << 32) - 1
    idx[bad[3]] = (idx[bad[3]] + 1) % 37  # another key's index
    want = b["want"].copy()
    want[bad] = 0
    with KC._keyset(engine, scheme, b) as ks:
        got = _wire_dev(engine, ks, b["sig"], idx, b["m"])
        assert (got == want).all(), _diff(got, want)
        assert (ks.verify_wire(b["sig"], idx, b["m"]) == want).all()


@pytest.mark.parametrize("scheme", SCHEMES)
def test_invalid_keys_give_zero(engine, scheme):
    b = _wire_batch(engine, scheme, 37, 4099)
    rec = b["rec"].copy()
    rec[3, :32] = np.frombuffer(M.le32(Q), np.uint8)  # v = q: from_bytes rejects the key
    P0 = b["P0"].copy()
    P0[5, 40] ^= 1                                     # off the curve
    under3, under5 = b["idx"] == 3, b["idx"] == 5
    assert (b["want"][under3] == 1).any() and (b["want"][under5] == 1).any()
    with engine.KeySet.from_wire(scheme, rec) as kw:
        assert kw.key_ok()[3] == 0 and kw.key_ok().sum() == 36
        want = b["want"].copy()
        want[under3] = 0
        got = _wire_dev(engine, kw, b["sig"], b["idx"], b["m"])
        assert (got == want).all(), _diff(got, want)
        assert (kw.verify_wire(b["sig"], b["idx"], b["m"]) == want).all()
        # ... which is the oracle's verdict on the undecodable key record
        assert (_oracle_wire(scheme, b["sig"], rec[b["idx"]], b["m"]) == want).all()
    with engine.KeySet(scheme, P0, b["P1"]) as ka:
        assert ka.key_ok()[5] == 0 and ka.key_ok().sum() == 36
        want = b["want"].copy()
        want[under5] = 0
        got = _wire_dev(engine, ka, b["sig"], b["idx"], b["m"])
        assert (got == want).all(), _diff(got, want)
        assert (ka.verify_wire(b["sig"], b["idx"], b["m"]) == want).all()


# ---- the _dev contract ------------------------------------------------------------------------------------
def test_dev_semantics(engine):
    from schnorr_amd import _lib

    L = _lib.load()
    n = 4099
    b = _wire_batch(engine, "single", 37, n)
    dsig, didx, dm = _to_dev(b["sig"]), _to_dev(b["idx"]), _to_dev(b["m"])
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    with KC._keyset(engine, "single", b) as ks:
        need = engine.keyed_wire_workspace_bytes("single", n)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        # enqueued on a side stream behind a poison fill on that stream
        side = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(side):
            ok = torch.empty(n, dtype=torch.uint8, device=DEV).fill_(POISON)
            ks.verify_wire_dev(dsig, didx, dm, ok, ws, stream=side)
        side.synchronize()
        assert (ok.cpu().numpy() == b["want"]).all()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        fn = L.dsv_verify_single_keyed_wire_dev
        call = lambda f, sigp, idxp, mp, nn, okt, wst, wsb: f(
            ks._h, sigp, idxp, mp, ctypes.c_size_t(nn), vp(okt) if okt is not None else None,
            vp(wst) if wst is not None else None, ctypes.c_size_t(wsb), stream)
        ok = _poison(n)
        # a workspace one byte short
        assert call(fn, vp(dsig), vp(didx), vp(dm), n, ok, ws, need - 1) == -2
        # a key set of another scheme
        assert call(L.dsv_verify_vargen_keyed_wire_dev, vp(dsig), vp(didx), vp(dm), n, ok, ws, need) == -2
        big = torch.empty(engine.keyed_wire_workspace_bytes("double", n), dtype=torch.uint8, device=DEV)
        sig96 = torch.zeros((n, 96), dtype=torch.uint8, device=DEV)
        assert call(L.dsv_verify_double_keyed_wire_dev, vp(sig96), vp(didx), vp(dm), n, ok, big, big.numel()) == -2
        # NULL pointers with n > 0
        assert call(fn, None, vp(didx), vp(dm), n, ok, ws, need) == -2
        assert call(fn, vp(dsig), None, vp(dm), n, ok, ws, need) == -2
        assert call(fn, vp(dsig), vp(didx), None, n, ok, ws, need) == -2
        assert call(fn, vp(dsig), vp(didx), vp(dm), n, None, ws, need) == -2
        assert call(fn, vp(dsig), vp(didx), vp(dm), n, ok, None, need) == -2
        # records not 16-byte aligned
        flat = torch.zeros(n * 64 + 64, dtype=torch.uint8, device=DEV)
        flat[8:8 + n * 64] = dsig.reshape(-1)
        assert (flat.data_ptr() + 8) % 16 == 8
        assert call(fn, ctypes.c_void_p(flat.data_ptr() + 8), vp(didx), vp(dm), n, ok, ws, need) == -2
        assert b"16-byte aligned" in L.dsv_last_error()
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == POISON).all()  # nothing was launched by any of them
        # n = 0
        assert call(fn, vp(dsig), vp(didx), vp(dm), 0, ok, ws, 0) == 0
        assert call(fn, None, None, None, 0, None, None, 0) == 0
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == POISON).all()
        # the exact workspace is enough
        assert call(fn, vp(dsig), vp(didx), vp(dm), n, ok, ws, need) == 0
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == b["want"]).all()
        with pytest.raises(ValueError):
            ks.verify_wire_dev(dsig, didx, dm, ok, ws[:need - 1])
        with pytest.raises(ValueError):
            ks.verify_wire_dev(sig96, didx, dm, ok, big)        # a double record on a single key set
        with pytest.raises(ValueError):
            ks.verify_wire_dev(dsig, didx[:-1], dm, ok, ws)
        with pytest.raises(ValueError):
            ks.verify_wire_dev(dsig, didx, dm, ok[:-1], ws)


# ---- host form = device form at the host pipeline's edges -------------------------------------------------
HOST_CASES = [(s, n) for s in SCHEMES for n in D.edges("host/wire/%s" % s)]
_HOST = {}


def _host_batch(engine, scheme):
    """one seeded, honest batch of the largest host size (sliced for the others), its key set's points"""
    if scheme not in _HOST:
        _HOST.clear()
        nmax, k = max(D.edges("host/wire/%s" % scheme)), 37
        assert nmax <= D.HOST_MAX
        sk, gen, P0, P1 = KC._keys(engine, scheme, k, 777)
        rng = np.random.default_rng(20261016)
        idx = rng.integers(0, k, size=nmax).astype(np.uint32)
        m = KC._scalars(rng, nmax, 0x3F)
        r = KC._scalars(rng, nmax, 0x07)
        Rp = None
        if scheme == "single":
            u, R = engine.sign_single(sk[idx], m, r)
        elif scheme == "double":
            u, R, Rp = engine.sign_double(sk[idx], m, r)
        else:
            u, R = engine.sign_vargen(sk[idx], gen[idx], m, r)
        _HOST[scheme] = {"sig": _sig(u, R, Rp), "idx": idx, "m": m, "ks": engine.KeySet(scheme, P0, P1)}
    return _HOST[scheme]


@pytest.mark.parametrize("scheme,n", HOST_CASES, ids=["%s-%d" % c for c in HOST_CASES])
def test_host_form_equals_dev_form_at_every_edge(engine, scheme, n):
    b = _host_batch(engine, scheme)
    sig, idx, m = b["sig"][:n].copy(), b["idx"][:n], b["m"][:n]
    # a wrong item at the first item of every sub-batch, whichever plan the call takes
    pos = sorted(set(D.host_parts(n, False)) | set(D.host_parts(n, True)))
    assert pos[0] == 0 and pos[-1] < n
    sig[pos, 0] ^= 1  # u + 1 or u - 1
    dev = _wire_dev(engine, b["ks"], sig, idx, m)
    # every item of the batch is honest, so the device form's zeros are exactly the planted ones
    assert np.array_equal(np.flatnonzero(dev == 0), np.array(pos)), (np.flatnonzero(dev == 0)[:8], pos[:8])
    host = b["ks"].verify_wire(sig, idx, m)
    assert np.array_equal(host, dev), _diff(host, dev)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_two_host_calls_in_flight(engine, scheme):
    b = _host_batch(engine, scheme)
    n = len(b["m"])
    sig = b["sig"].copy()
    sig[::11, 0] ^= 1
    dev = _wire_dev(engine, b["ks"], sig, b["idx"], b["m"])
    assert 0 < dev.sum() < n
    out, err = [None, None], []

    def work(t):
        try:
            lo = 0 if t == 0 else 12345
            for _ in range(3):
                out[t] = (lo, b["ks"].verify_wire(sig[lo:], b["idx"][lo:], b["m"][lo:]))
        except Exception as e:  # noqa: BLE001
            err.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    for lo, got in out:
        assert np.array_equal(got, dev[lo:]), _diff(got, dev[lo:])
    if scheme == SCHEMES[-1]:
        for v in _HOST.values():
            v["ks"].close()
        _HOST.clear()


# ---- lifetime ---------------------------------------------------------------------------------------------
def test_closed_set_raises(engine):
    b = _wire_batch(engine, "single", 37, 4099)
    ks = KC._keyset(engine, "single", b)
    assert (ks.verify_wire(b["sig"], b["idx"], b["m"]) == b["want"]).all()
    ks.close()
    with pytest.raises(ValueError):
        ks.verify_wire(b["sig"], b["idx"], b["m"])
    dsig, didx, dm = _to_dev(b["sig"]), _to_dev(b["idx"]), _to_dev(b["m"])
    ok = _poison(4099)
    ws = torch.empty(engine.keyed_wire_workspace_bytes("single", 4099), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        ks.verify_wire_dev(dsig, didx, dm, ok, ws)
    torch.cuda.synchronize()
    assert (ok.cpu().numpy() == POISON).all()


def test_shutdown_kills_the_wire_calls():
    """a process of its own (the session's engine stays up): after dsv_shutdown the host and device forms on
    a set that was live return DSV_ERR_NOT_INITIALIZED"""
    code = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import torch
from schnorr_amd import engine as E, _lib
E.init(0)
L = _lib.load()
sk = np.zeros((2, 32), np.uint8); sk[:, 0] = (3, 5)
pk = E.public_keys(sk)
m = np.zeros((2, 32), np.uint8); m[:, 0] = (9, 11)
r = np.zeros((2, 32), np.uint8); r[:, 0] = (21, 23)
u, R = E.sign_single(sk, m, r)
sig = np.ascontiguousarray(np.hstack([u, E.compress_points(R)]))
idx = np.arange(2, dtype=np.uint32)
ks = E.KeySet("single", pk)
assert list(ks.verify_wire(sig, idx, m)) == [1, 1]
assert list(ks.verify_wire(sig, idx[::-1].copy(), m)) == [0, 0]
E.shutdown()
h = ks._h
ok = np.full(2, 7, np.uint8)
p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
assert L.dsv_verify_single_keyed_wire(h, p(sig), p(idx), p(m), ctypes.c_size_t(2), p(ok)) == -1
assert L.dsv_verify_single_keyed_wire_dev(h, p(sig), p(idx), p(m), ctypes.c_size_t(2), p(ok), p(ok),
                                          ctypes.c_size_t(1 << 20), None) == -1
assert (ok == 7).all()
ks.close()
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
