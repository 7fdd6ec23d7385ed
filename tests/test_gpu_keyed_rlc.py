"""The keyed fast accept on the GPU (KeySet.verify_rlc_dev, dsv_verify_*_keyed_rlc_dev): whole verdict vectors
against the oracle and against the keyed per-signature path (KeySet.verify_dev) — all valid, one wrong
signature in forced sub-groups, malformed items, order-8 components in keys and nonce points, 2^20 items,
small batches, both kinds of `accepted` target, two streams, the keyed history counter, argument errors and
the refusal of graph capture (keyed and unkeyed device-pointer forms)."""
import ctypes
import random

import numpy as np
import pytest
import torch

import oracle_lib as O
import pymodel as M
import keyed_cases as KC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCHEMES = ("single", "double", "vargen")
MIN_AUTO = {"single": 1 << 19, "double": 1 << 19, "vargen": 1 << 19}
DSV_ERR_INVALID_ARGUMENT = -2

_BATCHES = {}


def _signed(engine, scheme, k, n, seed=0):
    """n VALID items under k keys (uniform indices): dict of key arrays P0 / P1 and items u, R, Rp, idx, m"""
    key = (scheme, k, n, seed)
    if key in _BATCHES:
        return {a: (v.copy() if isinstance(v, np.ndarray) else v) for a, v in _BATCHES[key].items()}
    sk, gen, P0, P1 = KC._keys(engine, scheme, k, 5000 + 17 * k + seed)
    rng = np.random.default_rng(n * 7 + k + seed)
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
    out = {"P0": P0, "P1": P1, "u": u, "R": R, "Rp": Rp, "idx": idx, "m": m}
    if len(_BATCHES) > 3:
        _BATCHES.pop(next(iter(_BATCHES)))
    _BATCHES[key] = out
    return {a: (v.copy() if isinstance(v, np.ndarray) else v) for a, v in out.items()}


def _set(engine, scheme, b):
    return engine.KeySet(scheme, b["P0"], b["P1"]) if scheme != "single" else engine.KeySet(scheme, b["P0"])


def _args(b):
    pts = [b["R"]] + ([b["Rp"]] if b["Rp"] is not None else [])
    return KC._dev([b["u"]] + pts + [b["idx"], b["m"]])


def _rlc(engine, ks, b, window_bits=0, stream=None, accepted_out=None):
    d = _args(b)
    n = b["u"].shape[0]
    ok = torch.full((max(n, 1),), 7, dtype=torch.uint8, device=DEV)
    ws = torch.empty(engine.keyed_rlc_workspace_bytes(n, ks.k, window_bits), dtype=torch.uint8, device=DEV)
    acc = ks.verify_rlc_dev(*d, ok[:n], ws, stream=stream, window_bits=window_bits, accepted_out=accepted_out)
    torch.cuda.synchronize()
    return acc, ok[:n].cpu().numpy()


def _per_sig(engine, ks, b):
    n = b["u"].shape[0]
    return KC._run_dev(engine, ks, _args(b), n)


def _oracle(scheme, b):
    g1 = b["P1"][b["idx"]] if b["P1"] is not None else None
    return KC._oracle(scheme, b["u"], b["R"], b["Rp"], b["P0"][b["idx"]], g1, b["m"])


def _wrong(b, i):
    """item i becomes a WRONG signature: u + 1 (still < r)"""
    u = M.from_le(bytes(b["u"][i]))
    b["u"][i] = np.frombuffer(M.le32((u + 1) % M.R_ORDER), np.uint8)


@pytest.fixture
def subgroups(engine):
    before = engine.rlc_subgroups(-1)
    yield engine.rlc_subgroups
    engine.rlc_subgroups(before)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_all_valid_is_accepted(engine, scheme):
    for k in (1, 3, 64):
        for bits in (0, 8, 12, 16):
            n = MIN_AUTO[scheme] if bits == 0 else 1500
            b = _signed(engine, scheme, k, n)
            with _set(engine, scheme, b) as ks:
                acc, ok = _rlc(engine, ks, b, bits)
                assert acc is True, (scheme, k, bits)
                assert ok.all(), KC._diff(ok, np.ones(n, np.uint8))
    b = _signed(engine, scheme, 3, 1500)
    with _set(engine, scheme, b) as ks:
        assert np.array_equal(_rlc(engine, ks, b, 8)[1], _per_sig(engine, ks, b))


@pytest.mark.parametrize("scheme", SCHEMES)
def test_one_wrong_signature_in_forced_sub_groups(engine, scheme, subgroups):
    n = 5000
    for groups, wrong in ((1, [77]), (2, [10, 4990]), (16, [3, 2600, 4999])):
        b = _signed(engine, scheme, 5, n)
        for i in wrong:
            _wrong(b, i)
        want = _oracle(scheme, b)
        assert want.sum() == n - len(wrong)
        subgroups(groups)
        with _set(engine, scheme, b) as ks:
            acc, ok = _rlc(engine, ks, b, 8)
            assert acc is False, (scheme, groups)
            assert np.array_equal(ok, want), KC._diff(ok, want)
            assert np.array_equal(ok, _per_sig(engine, ks, b))


@pytest.mark.parametrize("scheme", SCHEMES)
def test_malformed_items_stay_out_of_the_sum(engine, scheme):
    n = 1200
    b = _signed(engine, scheme, 4, n)
    top = np.frombuffer(b"\xff" * 32, np.uint8)
    b["u"][5] = top                      # u >= r
    b["R"][60, 32:] = top                # a coordinate >= q
    b["m"][1100] = top                   # m >= q
    b["idx"][300] = 4                    # idx >= k
    b["idx"][301] = 0xFFFFFFFF
    bad_key = b["P0"].copy()
    bad_key[3, :32] = top                # key 3: a coordinate >= q -> key_ok = 0
    b2 = dict(b, P0=bad_key)
    with _set(engine, scheme, b2) as ks:
        assert list(ks.key_ok()) == [1, 1, 1, 0]
        under_bad = b["idx"] == 3
        acc, ok = _rlc(engine, ks, b2, 8)
        want = np.ones(n, np.uint8)
        want[[5, 60, 1100, 300, 301]] = 0
        want[under_bad] = 0
        assert np.array_equal(ok, want), KC._diff(ok, want)
        assert acc is True
        assert np.array_equal(ok, _per_sig(engine, ks, b2))


def _torsion_items(engine, count, cancel, key_torsion, rnd):
    """single-scheme items whose key (key_torsion) or nonce point carries an order-8 component; cancel: valid
    under the reference's cofactorless equation.  Returns (PK rows, u, R, m)."""
    import torsion_model as TM

    t8 = TM.order8_point()
    rows = {"PK": [], "u": [], "R": [], "m": []}
    while len(rows["u"]) < count:
        sk, m, rr = rnd.randrange(1, M.R_ORDER), rnd.randrange(M.Q), rnd.randrange(1, M.R_ORDER)
        k1 = rnd.randrange(1, 8) if key_torsion else 0
        k2 = rnd.randrange(8) if key_torsion else rnd.randrange(1, 8)
        pk = M.padd(M.pmul(M.GEN, sk), M.pmul(t8, k1))
        R = M.padd(M.pmul(M.GEN, rr), M.pmul(t8, k2))
        c = M.challenge(R, m)
        if ((c * k1 - k2) % 8 == 0) != cancel:
            continue
        rows["u"].append(np.frombuffer(M.le32((rr - c * sk) % M.R_ORDER), np.uint8))
        rows["R"].append(np.frombuffer(M.point_bytes(R), np.uint8))
        rows["PK"].append(np.frombuffer(M.point_bytes(pk), np.uint8))
        rows["m"].append(np.frombuffer(M.le32(m), np.uint8))
    return {a: np.stack(v) for a, v in rows.items()}


def test_order8_components_are_never_accepted(engine):
    rnd = random.Random(8)
    n = 900
    for key_torsion, cancel in ((True, True), (True, False), (False, False)):
        b = _signed(engine, "single", 6, n)
        t = _torsion_items(engine, 2, cancel, key_torsion, rnd)
        k0 = b["P0"].shape[0]
        b["P0"] = np.concatenate([b["P0"], t["PK"]])
        for j, at in enumerate((100, 700)):
            b["u"][at], b["R"][at], b["m"][at] = t["u"][j], t["R"][j], t["m"][j]
            b["idx"][at] = k0 + j
        want = _oracle("single", b)
        with _set(engine, "single", b) as ks:
            acc, ok = _rlc(engine, ks, b, 8)
            assert acc is False, (key_torsion, cancel)
            assert np.array_equal(ok, want), KC._diff(ok, want)
            assert np.array_equal(ok, _per_sig(engine, ks, b))


def test_an_unreferenced_torsion_key_is_still_accepted(engine):
    rnd = random.Random(9)
    b = _signed(engine, "single", 6, 900)
    t = _torsion_items(engine, 1, True, True, rnd)
    b["P0"] = np.concatenate([b["P0"], t["PK"]])   # key 6: order-8 component, no item under it
    with _set(engine, "single", b) as ks:
        acc, ok = _rlc(engine, ks, b, 8)
        assert acc is True and ok.all()


@pytest.mark.parametrize("scheme,k", [("single", 64), ("single", 1), ("double", 64), ("vargen", 64)])
def test_2p20_items(engine, scheme, k):
    n = 1 << 20
    b = _signed(engine, scheme, k, n)
    with _set(engine, scheme, b) as ks:
        acc, ok = _rlc(engine, ks, b)
        assert acc is True and ok.all()
        if scheme == "single" and k == 64:
            _wrong(b, 777777)
            want = _per_sig(engine, ks, b)
            assert want.sum() == n - 1 and want[777777] == 0
            acc, ok = _rlc(engine, ks, b)
            assert acc is False
            assert np.array_equal(ok, want), KC._diff(ok, want)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_small_batches(engine, scheme):
    t = MIN_AUTO[scheme]
    for n in (1, t - 1, t):
        b = _signed(engine, scheme, 3, n)
        with _set(engine, scheme, b) as ks:
            acc, ok = _rlc(engine, ks, b)
            assert ok.all(), (scheme, n)
            assert acc is (n >= t), (scheme, n)   # below the threshold: the per-signature kernel, not accepted
    from schnorr_amd import _lib

    b = _signed(engine, scheme, 3, 1)
    with _set(engine, scheme, b) as ks:   # n = 0: DSV_OK, nothing written but `accepted` = 0
        d = _args(b)
        ok = torch.full((1,), 7, dtype=torch.uint8, device=DEV)
        acc = ctypes.c_int(5)
        rc = getattr(_lib.load(), "dsv_verify_%s_keyed_rlc_dev" % scheme)(
            ks._handle(), *[ctypes.c_void_p(t.data_ptr()) for t in d], ctypes.c_size_t(0), ctypes.c_void_p(ok.data_ptr()),
            ctypes.c_void_p(ok.data_ptr()), ctypes.c_size_t(0), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
            ctypes.c_int(0), ctypes.byref(acc))
        torch.cuda.synchronize()
        assert rc == 0 and acc.value == 0 and ok.item() == 7


def test_accepted_targets(engine):
    b = _signed(engine, "single", 3, 1500)
    with _set(engine, "single", b) as ks:
        dev = torch.zeros(1, dtype=torch.int32, device=DEV)
        assert _rlc(engine, ks, b, 8, accepted_out=dev)[0] is None and dev.item() == 1
        pinned = torch.zeros(1, dtype=torch.int32).pin_memory()
        assert _rlc(engine, ks, b, 8, accepted_out=pinned)[0] is None and pinned.item() == 1
        assert _rlc(engine, ks, b, 8)[0] is True
        _wrong(b, 9)
        dev.fill_(1)
        assert _rlc(engine, ks, b, 8, accepted_out=dev)[0] is None and dev.item() == 0


def test_two_streams_one_set(engine):
    b1 = _signed(engine, "double", 5, 3000, seed=1)
    b2 = _signed(engine, "double", 5, 3000, seed=1)
    _wrong(b2, 1234)
    with _set(engine, "double", b1) as ks:
        want = [_per_sig(engine, ks, b1), _per_sig(engine, ks, b2)]
        s = [torch.cuda.Stream(), torch.cuda.Stream()]
        oks, accs = [], []
        for b, st in zip((b1, b2), s):
            d = _args(b)
            ok = torch.full((3000,), 7, dtype=torch.uint8, device=DEV)
            ws = torch.empty(engine.keyed_rlc_workspace_bytes(3000, ks.k, 8), dtype=torch.uint8, device=DEV)
            acc = torch.zeros(1, dtype=torch.int32, device=DEV)
            torch.cuda.current_stream().synchronize()
            ks.verify_rlc_dev(*d, ok, ws, stream=st, window_bits=8, accepted_out=acc)
            oks.append((ok, ws, d))
            accs.append(acc)
        torch.cuda.synchronize()
        assert np.array_equal(oks[0][0].cpu().numpy(), want[0])
        assert np.array_equal(oks[1][0].cpu().numpy(), want[1])
        assert [a.item() for a in accs] == [1, 0]


def test_keyed_history_is_its_own(engine):
    b = _signed(engine, "single", 3, 1500)
    _wrong(b, 3)
    with _set(engine, "single", b) as ks:
        engine.keyed_rlc_history(0, 0)
        unkeyed = engine.rlc_history(0, 3)
        unkeyed_long = engine.rlc_history_long(0, 5)
        acc, ok = _rlc(engine, ks, b, 8)
        assert acc is False and ok.sum() == 1499
        assert engine.rlc_history(0) == 3 and engine.rlc_history_long(0) == 5
        assert engine.keyed_rlc_history(0) == 8
        engine.rlc_history(0, unkeyed)
        engine.rlc_history_long(0, unkeyed_long)
        engine.keyed_rlc_history(0, 0)


def test_argument_errors_launch_nothing(engine):
    from schnorr_amd import _lib

    L = _lib.load()
    b = _signed(engine, "single", 3, 1000)
    with _set(engine, "single", b) as ks, _set(engine, "double", _signed(engine, "double", 2, 10)) as other:
        d = _args(b)
        ok = torch.full((1000,), 7, dtype=torch.uint8, device=DEV)
        need = engine.keyed_rlc_workspace_bytes(1000, ks.k, 8)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        p = [ctypes.c_void_p(t.data_ptr()) for t in d]
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        acc = ctypes.c_int(5)
        call = L.dsv_verify_single_keyed_rlc_dev
        rc = call(ks._handle(), *p, ctypes.c_size_t(1000), ctypes.c_void_p(ok.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                  ctypes.c_size_t(need - 256), s, ctypes.c_int(8), ctypes.byref(acc))
        assert rc == DSV_ERR_INVALID_ARGUMENT
        rc = call(other._handle(), *p, ctypes.c_size_t(1000), ctypes.c_void_p(ok.data_ptr()),
                  ctypes.c_void_p(ws.data_ptr()), ctypes.c_size_t(need), s, ctypes.c_int(8), ctypes.byref(acc))
        assert rc == DSV_ERR_INVALID_ARGUMENT
        rc = call(ks._handle(), *p, ctypes.c_size_t(1000), ctypes.c_void_p(ok.data_ptr()), ctypes.c_void_p(ws.data_ptr()),
                  ctypes.c_size_t(need), s, ctypes.c_int(10), ctypes.byref(acc))
        assert rc == DSV_ERR_INVALID_ARGUMENT
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == 7).all() and acc.value == 5


def test_capture_is_refused(engine):
    from schnorr_amd import _lib

    b = _signed(engine, "single", 3, 1000)
    with _set(engine, "single", b) as ks:
        d = _args(b)
        ok = torch.full((1000,), 7, dtype=torch.uint8, device=DEV)
        ws = torch.empty(engine.keyed_rlc_workspace_bytes(1000, ks.k, 8), dtype=torch.uint8, device=DEV)
        acc = torch.zeros(1, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            twice = ok.to(torch.int32) * 2  # (a node of its own: the capture is not empty)
            with pytest.raises(_lib.DsvError):
                ks.verify_rlc_dev(*d, ok, ws, window_bits=8, accepted_out=acc)
        del g, twice  # ended, never replayed
        torch.cuda.synchronize()
        assert (ok.cpu().numpy() == 7).all()
        # the same call outside a capture works
        assert _rlc(engine, ks, b, 8)[0] is True


@pytest.mark.parametrize("form", ["single", "wire", "mixed"])
def test_capture_is_refused_unkeyed(engine, form):
    """the unkeyed device-pointer fast accepts (affine, wire records, mixed batch) draw their weights on the host
    per call too: a capturing stream is refused as the keyed form refuses it"""
    from schnorr_amd import _lib

    b = _signed(engine, "single", 3, 1000)
    n, PK = len(b["m"]), b["P0"][b["idx"]]
    if form == "wire":
        cp = engine.compress_points
        args = KC._dev([np.concatenate([b["u"], cp(b["R"])], axis=1), cp(PK), b["m"]])
        ws = torch.empty(engine.wire_rlc_workspace_bytes(n, 8), dtype=torch.uint8, device=DEV)
        call = lambda ok: engine.verify_wire_rlc_dev("single", *args, ok, ws, window_bits=8)
    elif form == "mixed":
        u, R, PKt, m = KC._dev([b["u"], b["R"], PK, b["m"]])
        kinds = torch.zeros(n, dtype=torch.uint8, device=DEV)
        ws = torch.empty(engine.mixed_rlc_workspace_bytes(n), dtype=torch.uint8, device=DEV)
        call = lambda ok: engine.verify_mixed_rlc_dev(kinds, u, R, R, PKt, PKt, m, 0, ok, ws)
    else:
        args = KC._dev([b["u"], b["R"], PK, b["m"]])
        ws = torch.empty(engine.rlc_workspace_bytes(n, 8), dtype=torch.uint8, device=DEV)
        call = lambda ok: engine.verify_single_rlc_dev(*args, ok, ws, window_bits=8)
    ok = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        twice = ok.to(torch.int32) * 2  # (a node of its own: the capture is not empty)
        with pytest.raises(_lib.DsvError):
            call(ok)
    del g, twice  # ended, never replayed
    torch.cuda.synchronize()
    assert (ok.cpu().numpy() == 7).all()
    # the same call outside a capture works (mixed: automatic window bits, below the aggregate's threshold)
    accepted = call(ok)
    torch.cuda.synchronize()
    assert (ok.cpu().numpy() == 1).all()
    assert accepted is (form != "mixed")
