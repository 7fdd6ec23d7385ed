"""Registered key sets on the GPU (dsv_keyset_*, dsv_verify_*_keyed*): whole-vector parity with the oracle on
the gathered keys for all three schemes, adversarial base sets registered by unique key, 2^20 items against
the unkeyed kernels, table entries against true multiples, key validity, index checks, the _dev contract,
lifetime, the host form and shutdown."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import edge_sets as ES
import harness as H
import oracle_lib as O
import pymodel as M
import torsion_model as TM
from keyed_cases import _batch, _dev, _diff, _items, _keys, _keyset, _oracle, _poison, _run_dev, _scalars

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEMES = ("single", "double", "vargen")
NS = (1, 63, 64, 65, 4099, (1 << 16) + 3)
Q, R_ORDER = M.Q, M.R_ORDER


# ---- oracle parity ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 37, 1000))
@pytest.mark.parametrize("scheme", SCHEMES)
def test_oracle_parity(engine, scheme, k):
    b = _batch(engine, scheme, k, NS[-1])
    assert 0 < b["want"].sum() < len(b["want"])
    with _keyset(engine, scheme, b) as ks:
        assert ks.k == k and ks.nbytes == engine.keyset_bytes(scheme, k)
        assert (ks.key_ok() == 1).all()
        darrs = _dev(_items(b))
        for n in NS:
            got = _run_dev(engine, ks, darrs, n)
            assert (got == b["want"][:n]).all(), (scheme, k, n, _diff(got, b["want"][:n]))


# ---- adversarial base sets, registered by unique key ------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_adversarial_base_set(engine, scheme):
    arrs, want = ES.base(scheme, "affine", "mixed")
    names = ES.FIELDS[scheme]
    d = dict(zip(names, arrs))
    second = {"single": None, "double": "PKp", "vargen": "Gen"}[scheme]
    rows = d["PK"] if second is None else np.hstack([d["PK"], d[second]])
    uniq, inv = np.unique(rows, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1).astype(np.uint32)
    P0 = np.ascontiguousarray(uniq[:, :64])
    P1 = np.ascontiguousarray(uniq[:, 64:]) if second else None
    items = [d["u"], d["R"]] + ([d["Rp"]] if scheme == "double" else []) + [inv, d["m"]]
    with engine.KeySet(scheme, P0, P1) as ks:
        got = _run_dev(engine, ks, _dev(items), len(want))
        assert (got == want).all(), _diff(got, want)
        assert (ks.verify(*items) == want).all()


# ---- 2^20 items against the unkeyed kernels ---------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_two_pow_20_matches_unkeyed(engine, scheme):
    n, k = 1 << 20, 64
    sk, gen, P0, P1 = _keys(engine, scheme, k, 4242)
    rng = np.random.default_rng(99)
    idx = rng.integers(0, k, size=n).astype(np.uint32)
    m = _scalars(rng, n, 0x3F)
    r = _scalars(rng, n, 0x07)
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
    items = [u, R] + ([Rp] if Rp is not None else []) + [idx, m]
    d = _dev(items)
    with engine.KeySet(scheme, P0, P1) as ks:
        got = _run_dev(engine, ks, d, n)
    g0, g1 = torch.from_numpy(P0[idx]).to(DEV), (torch.from_numpy(P1[idx]).to(DEV) if P1 is not None else None)
    ok = _poison(n)
    ws = torch.empty(engine.workspace_bytes(n), dtype=torch.uint8, device=DEV)
    du, dR, dm = d[0], d[1], d[-1]
    if scheme == "single":
        engine.verify_single_dev(du, dR, g0, dm, ok, ws)
    elif scheme == "double":
        engine.verify_double_dev(du, dR, d[2], g0, g1, dm, ok, ws)
    else:
        engine.verify_vargen_dev(du, dR, g0, g1, dm, ok, ws)
    torch.cuda.synchronize()
    ref = ok.cpu().numpy()
    assert (got == ref).all(), _diff(got, ref)
    assert 0.8 < got.mean() < 0.9
    sample = np.sort(rng.choice(n, 4096, replace=False))
    want = _oracle(scheme, u[sample], R[sample], Rp[sample] if Rp is not None else None, P0[idx[sample]],
                   P1[idx[sample]] if P1 is not None else None, m[sample])
    assert (got[sample] == want).all(), _diff(got[sample], want)


# ---- table entries ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("point", (0, 1))
def test_table_entries_are_true_multiples(engine, point):
    """entry [w][d] of a normal and a small-order (order 8) point equals d * 2^(8w) * P; -d its negation"""
    normal = H.to_int_point(engine.public_keys(_scalars(np.random.default_rng(5), 1, 0x07))[0])
    small = TM.order8_point()
    pts = [normal, small]
    P0 = np.stack([np.frombuffer(M.point_bytes(p), np.uint8) for p in pts])
    # point 1 (double: PK'): the same two points in the other slot, a different first point
    P1 = P0.copy()
    if point == 1:
        P0 = np.stack([np.frombuffer(M.point_bytes(M.pmul(M.GEN, 12345 + j)), np.uint8) for j in range(2)])
    scheme = "single" if point == 0 else "double"
    with engine.KeySet(scheme, P0, P1 if point == 1 else None) as ks:
        assert (ks.key_ok() == 1).all()
        for key, P in enumerate(pts):
            Pb = np.frombuffer(M.point_bytes(P), np.uint8).reshape(1, 64)
            for w in (0, 1, 15, 30, 31):
                for d in (0, 1, 2, 15, 32, 127, 128):
                    s = d << (8 * w)
                    if s < 1 << 252:
                        want = O.scalar_mul(np.frombuffer(M.le32(s), np.uint8).reshape(1, 32), Pb)[0]
                    else:
                        want = np.frombuffer(M.point_bytes(M.pmul(P, s)), np.uint8)
                    got = ks.debug_entry(key, point, w, d)
                    assert (got == want).all(), (key, w, d)
                    neg = np.frombuffer(M.point_bytes(M.pneg(H.to_int_point(want))), np.uint8)
                    assert (ks.debug_entry(key, point, w, -d) == neg).all(), (key, w, -d)


# ---- key validity -----------------------------------------------------------------------------------------
def test_invalid_keys_and_wire_form(engine):
    b = _batch(engine, "single", 37, 4099)
    P0 = b["P0"].copy()
    pk1 = H.to_int_point(P0[1])
    if pk1[0] + Q < 1 << 256:
        P0[1, :32] = np.frombuffer(M.le32(pk1[0] + Q), np.uint8)  # u >= q, same residue
    else:
        P0[1, :32] = 0xFF
    P0[2, 40] ^= 1                                                # v changed: off the curve
    assert not M.on_curve(H.to_int_point(P0[2]))
    items = _items(b)
    idx = b["idx"]
    with engine.KeySet("single", P0) as ks:
        kok = ks.key_ok()
        assert kok[1] == 0 and kok[2] == 0 and kok.sum() == 35
        got = ks.verify(*items)
    bad = np.isin(idx, (1, 2))
    assert bad.sum() > 0 and (got[bad] == 0).all()
    assert (got[~bad] == b["want"][~bad]).all(), _diff(got[~bad], b["want"][~bad])
    # wire records: the same verdicts as the affine set; an undecodable record is an invalid key
    for scheme in SCHEMES:
        bs = _batch(engine, scheme, 37, 4099)
        rec = O.compress(bs["P0"]) if scheme == "single" else np.hstack([O.compress(bs["P0"]), O.compress(bs["P1"])])
        rec = np.ascontiguousarray(rec)
        its = _items(bs)
        with engine.KeySet(scheme, bs["P0"], bs["P1"]) as ka, engine.KeySet.from_wire(scheme, rec) as kw:
            assert (kw.key_ok() == 1).all()
            va = ka.verify(*its)
            assert (va == bs["want"]).all(), _diff(va, bs["want"])
            assert (kw.verify(*its) == va).all()
        rec[3, :32] = np.frombuffer(M.le32(Q), np.uint8)  # v = q: from_bytes rejects it
        with engine.KeySet.from_wire(scheme, rec) as kw:
            kok = kw.key_ok()
            assert kok[3] == 0 and kok.sum() == 36
            got = kw.verify(*its)
            under = bs["idx"] == 3
            assert under.sum() > 0 and (got[under] == 0).all() and (got[~under] == va[~under]).all()


# ---- indices ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_index_checks(engine, scheme):
    b = _batch(engine, scheme, 37, 4099)
    items = _items(b)
    idx = b["idx"].copy()
    honest = np.flatnonzero(b["want"] == 1)
    bad = honest[:4]
    idx[bad[0]], idx[bad[1]], idx[bad[2]] = 37, 1 << 31, (1 << 32) - 1
    idx[bad[3]] = (idx[bad[3]] + 1) % 37  # another key's index
    items[-2] = idx
    want = b["want"].copy()
    want[bad] = 0
    with _keyset(engine, scheme, b) as ks:
        got = _run_dev(engine, ks, _dev(items), len(want))
        assert (got == want).all(), _diff(got, want)
        assert (ks.verify(*items) == want).all()


# ---- the _dev contract ------------------------------------------------------------------------------------
def test_dev_semantics(engine):
    from schnorr_amd import _lib

    L = _lib.load()
    b = _batch(engine, "single", 37, 4099)
    n = 4099
    du, dR, di, dm = _dev(_items(b))
    with _keyset(engine, "single", b) as ks:
        # enqueued on a side stream behind a poison fill on that stream
        side = torch.cuda.Stream(device=DEV)
        ws = torch.empty(engine.keyed_workspace_bytes(n), dtype=torch.uint8, device=DEV)
        with torch.cuda.stream(side):
            ok = torch.empty(n, dtype=torch.uint8, device=DEV).fill_(POISON)
            ks.verify_dev(du, dR, di, dm, ok, ws, stream=side)
        side.synchronize()
        assert (ok.cpu().numpy() == b["want"]).all()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        args = lambda nn, okt, wst, wsb: (ks._h, ctypes.c_void_p(du.data_ptr()), ctypes.c_void_p(dR.data_ptr()),
                                         ctypes.c_void_p(di.data_ptr()), ctypes.c_void_p(dm.data_ptr()),
                                         ctypes.c_size_t(nn), ctypes.c_void_p(okt.data_ptr()),
                                         ctypes.c_void_p(wst.data_ptr()), ctypes.c_size_t(wsb), stream)
        # a workspace one byte short: DSV_ERR_INVALID_ARGUMENT, nothing launched
        ok = _poison(n)
        assert L.dsv_verify_single_keyed_dev(*args(n, ok, ws, ws.numel() - 1)) == -2
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == POISON).all()
        # n = 0
        assert L.dsv_verify_single_keyed_dev(*args(0, ok, ws, 0)) == 0
        # a key set of the wrong scheme
        assert L.dsv_verify_vargen_keyed_dev(*args(n, ok, ws, ws.numel())) == -2
        dRp = dR.clone()
        assert L.dsv_verify_double_keyed_dev(ks._h, ctypes.c_void_p(du.data_ptr()), ctypes.c_void_p(dR.data_ptr()),
                                             ctypes.c_void_p(dRp.data_ptr()), ctypes.c_void_p(di.data_ptr()),
                                             ctypes.c_void_p(dm.data_ptr()), ctypes.c_size_t(n),
                                             ctypes.c_void_p(ok.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                                             ctypes.c_size_t(ws.numel()), stream) == -2
        # null pointer with n > 0
        assert L.dsv_verify_single_keyed_dev(ks._h, None, ctypes.c_void_p(dR.data_ptr()), ctypes.c_void_p(di.data_ptr()),
                                             ctypes.c_void_p(dm.data_ptr()), ctypes.c_size_t(n),
                                             ctypes.c_void_p(ok.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                                             ctypes.c_size_t(ws.numel()), stream) == -2
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == POISON).all()
        with pytest.raises(ValueError):
            ks.verify_dev(du, dR, dR, di, dm, ok, ws)  # double arguments on a single key set
        with pytest.raises(ValueError):
            ks.verify_dev(du, dR, di, dm, ok, ws[:10])


# ---- the constructors' contract ---------------------------------------------------------------------------
def _zeros_dev(nbytes):
    return torch.zeros(nbytes, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("scheme", (0, 1, 2))
@pytest.mark.parametrize("form", ("affine", "wire", "mont"))
def test_constructor_contract(engine, form, scheme):
    """dsv_keyset_create / _create_wire / _create_mont_cols through the C ABI: the order of the argument checks
    (output handle, scheme, key count, the form's pointers), and the empty set every form can build"""
    from schnorr_amd import _lib

    L = _lib.load()
    INVALID, TOO_LARGE = -2, -5
    np_keys = 1 if scheme == 0 else 2
    vp, sz, null = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p(None)
    host = np.zeros(2 * 96 * 2, np.uint8)  # a readable host buffer; no case below reads it
    hp = vp(host.ctypes.data)

    def create(sch, data, k, out):
        """data: the form's pointer arguments (affine: pk_uv, pk2_uv; wire: records; mont: cols)"""
        fn = {"affine": L.dsv_keyset_create, "wire": L.dsv_keyset_create_wire,
              "mont": L.dsv_keyset_create_mont_cols}[form]
        return fn(ctypes.c_int(sch), *data, sz(k), out)

    def cols(*pairs):
        return ((_lib.Column * 2)(*[_lib.Column(b, s) for b, s in pairs]),)

    no_data = {"affine": (null, null), "wire": (null,), "mont": (null,)}[form]
    h = vp(0xDEAD0)
    # null output handle
    assert create(scheme, no_data, 0, None) == INVALID
    # unknown scheme: the handle is cleared first
    assert create(3, no_data, 0, ctypes.byref(h)) == INVALID
    assert not h.value
    # the key count is checked before the pointers
    assert create(scheme, no_data, 1 << 32, ctypes.byref(h)) == TOO_LARGE
    # null data pointers with k > 0
    if form == "affine":
        bad = [((null, hp), None)] if scheme == 0 else [((hp, null), None)]
    elif form == "wire":
        bad = [((null,), None)]
    else:
        last = np_keys - 1  # the scheme's last key column ("column 1" for the two-point schemes)
        good = [(host.ctypes.data, 96)] * 2
        hole, short = list(good), list(good)
        hole[last] = (None, 96)
        short[last] = (host.ctypes.data, 95)
        bad = [((null,), None), (cols(*hole), "column %d" % last), (cols(*short), "stride")]
    for data, text in bad:
        h = vp(0xDEAD0)
        assert create(scheme, data, 2, ctypes.byref(h)) == INVALID, (form, scheme, text)
        assert not h.value
        if text:
            msg = L.dsv_last_error().decode()
            assert text in msg, msg
    # the empty set
    h = vp(0xDEAD0)
    assert create(scheme, no_data, 0, ctypes.byref(h)) == 0, L.dsv_last_error().decode()
    assert h.value and h.value != 0xDEAD0
    sch, k, nbytes, dev = ctypes.c_int(-1), sz(99), sz(99), ctypes.c_int(-1)
    assert L.dsv_keyset_info(h, ctypes.byref(sch), ctypes.byref(k), ctypes.byref(nbytes), ctypes.byref(dev)) == 0
    assert (sch.value, k.value, nbytes.value, dev.value) == (scheme, 0, 0, torch.cuda.current_device())
    assert L.dsv_keyset_key_ok(h, None) == 0
    # the form's per-signature _dev call on it: n = 0, then three items whose indices are all out of range
    n = 3
    ns = 2 if scheme == 1 else 1  # nonce points of a signature
    idx = torch.from_numpy(np.array([0, 1, 0xFFFFFFFF], np.uint32).view(np.int32)).to(DEV)
    m = _zeros_dev(n * 32)
    stream = vp(torch.cuda.current_stream().cuda_stream)
    p = lambda t: vp(t.data_ptr())
    if form == "affine":
        fn = (L.dsv_verify_single_keyed_dev, L.dsv_verify_double_keyed_dev, L.dsv_verify_vargen_keyed_dev)[scheme]
        u, pts = _zeros_dev(n * 32), [_zeros_dev(n * 64) for _ in range(ns)]
        ws_bytes = L.dsv_keyed_workspace_bytes(n)
        head = [h, p(u)] + [p(t) for t in pts] + [p(idx), p(m)]
    elif form == "wire":
        fn = (L.dsv_verify_single_keyed_wire_dev, L.dsv_verify_double_keyed_wire_dev,
              L.dsv_verify_vargen_keyed_wire_dev)[scheme]
        sig = _zeros_dev(n * (32 + 32 * ns))
        ws_bytes = L.dsv_keyed_wire_workspace_bytes(scheme, n)
        head = [h, p(sig), p(idx), p(m)]
    else:
        fn = L.dsv_verify_keyed_mont_dev
        u, R, Rp = _zeros_dev(n * 32), _zeros_dev(n * 96), _zeros_dev(n * 96)
        ws_bytes = L.dsv_keyed_mont_workspace_bytes(scheme, n)
        head = [h, p(u), p(R), p(Rp) if ns == 2 else null, p(idx), p(m)]
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    ok = _poison(n)
    assert fn(*head, sz(0), p(ok), p(ws), sz(ws_bytes), stream) == 0
    torch.cuda.synchronize()
    assert (ok.cpu().numpy() == POISON).all()
    assert fn(*head, sz(n), p(ok), p(ws), sz(ws_bytes), stream) == 0, L.dsv_last_error().decode()
    torch.cuda.synchronize()
    assert ok.cpu().numpy().tolist() == [0, 0, 0]
    assert L.dsv_keyset_destroy(h) == 0


# ---- lifetime ---------------------------------------------------------------------------------------------
def test_lifetime(engine):
    b1 = _batch(engine, "single", 37, 4099)
    b2 = _batch(engine, "vargen", 37, 4099)
    ks1, ks2 = _keyset(engine, "single", b1), _keyset(engine, "vargen", b2)
    assert (ks1.verify(*_items(b1)) == b1["want"]).all()
    ks1.close()
    ks1.close()  # idempotent
    assert (ks2.verify(*_items(b2)) == b2["want"]).all()
    with pytest.raises(ValueError):
        ks1.verify(*_items(b1))
    ks2.close()
    torch.cuda.synchronize()
    pk = b1["P0"]
    big = np.tile(pk, (3, 1))[:100]
    with engine.KeySet("single", big):
        pass
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(10):
        ks = engine.KeySet("single", big)
        assert ks.nbytes > 50 << 20
        ks.close()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < 32 << 20, (free0, free1)


# ---- host form --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_host_form_equals_dev_form(engine, scheme):
    b = _batch(engine, scheme, 37, NS[-1])
    n = (1 << 18) + 5
    reps = -(-n // NS[-1])
    items = [np.concatenate([a] * reps)[:n] for a in _items(b)]
    with _keyset(engine, scheme, b) as ks:
        host = ks.verify(*items)
        dev = _run_dev(engine, ks, _dev(items), n)
    want = np.tile(b["want"], reps)[:n]
    assert (host == dev).all(), _diff(host, dev)
    assert (host == want).all(), _diff(host, want)


# ---- shutdown (a process of its own: the session's engine stays up) ----------------------------------------
def test_shutdown_kills_live_sets():
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
ks = E.KeySet("single", pk)
assert list(ks.key_ok()) == [1, 1]
E.shutdown()
h = ks._h
u = np.zeros((1, 32), np.uint8); R = np.zeros((1, 64), np.uint8); idx = np.zeros(1, np.uint32); ok = np.zeros(1, np.uint8)
p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
assert L.dsv_verify_single_keyed(h, p(u), p(R), p(idx), p(u), ctypes.c_size_t(1), p(ok)) == -1
assert L.dsv_keyset_key_ok(h, p(ok)) == -1
ks.close()  # dsv_keyset_destroy on a dead set: DSV_OK
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
