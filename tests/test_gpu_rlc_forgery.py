"""The batch fast accept must reject forgeries that CANCEL under equal or structured weights (GPU).

Every other test of the fast accept plants one defect per aggregate, and z d != O for any non-zero weight:
they say nothing about the weights beyond "not zero".  (A constant z = 1 they do notice, by accident: equal
digits overflow the bins from 12-bit windows on, and 22 of the 32 tests of tests/test_gpu_rlc.py fail; at 8-bit
windows equal weights pass them, and non-zero but structured weights — a range-local counter, z' == z, few
effective bits — reject a single defect as surely as proper ones do.)  The batches here (tests/forgery_sets.py; the oracle-side conditions
are checked on the CPU in tests/test_forgery_sets.py) hold two wrong items — or one double-scheme item with
both equations off — whose defects sum to the identity when weighted equally: a constant z, two items
drawing the same keystream block (a range-local counter), z' == z, all accept them.  Through the public
entry points only, with the history counters at 0 and no forced sub-groups before every call, so that ONE
aggregate over the whole batch decides (no sample pre-check, no split that separates the pair).

For every batch: not accepted, the verdicts are the oracle's (zero on exactly the forged items), and — the
control — the same batch with the forgery undone is accepted under the same settings.
"""
import contextlib

import numpy as np
import pytest
import torch

import dispatch_edges as D
import forgery_sets as F
import mont_cases as C
import oracle_lib as O
from gpu_cases import _dev_col

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCHEMES = ("single", "double", "vargen")
N = F.N
BITS = (8, 12)   # fine bins only, kmul = 17; coarse bins, kmul = 1
# Smallest group that runs an aggregate with automatic window bits, device-resident forms (rlc.h: rlc_min_auto),
# read from the sources as tests/dispatch_edges.py reads them: a threshold that moves takes these sizes with it
# (or fails tests/test_dispatch_edges.py), and tests/test_gpu_dispatch_edges.py shows that one item fewer runs none.
MIN_AUTO = {"single": D.constants()["kRlcMinAuto"], "double": D._pinned("rlc_min_auto")[0]}


@contextlib.contextmanager
def one_aggregate(engine):
    """-> arm(groups=0): history counters 0, `groups` forced sub-groups — called before every call; everything
    restored at the end"""
    saved = (engine.rlc_history(0), engine.rlc_history_long(0), engine.keyed_rlc_history(0), engine.rlc_subgroups(-1))

    def arm(groups=0):
        engine.rlc_history(0, 0)
        engine.rlc_history_long(0, 0)
        engine.keyed_rlc_history(0, 0)
        engine.rlc_subgroups(groups)

    try:
        yield arm
    finally:
        engine.rlc_history(0, saved[0])
        engine.rlc_history_long(0, saved[1])
        engine.keyed_rlc_history(0, saved[2])
        engine.rlc_subgroups(saved[3])


_FORGED = {}


def forged(scheme, kind, pair):
    """(Forgery over the 1543-item base, the oracle's verdicts on its forged batch), built once"""
    key = (scheme, kind, pair)
    if key not in _FORGED:
        f = F.forge(scheme, kind, pair)
        want = F.oracle(scheme, f.forged)
        expect = np.ones(N, np.uint8)
        expect[f.items] = 0
        assert np.array_equal(want, expect)
        _FORGED[key] = (f, want)
    return _FORGED[key]


def _run_dev(engine, arm, scheme, a, bits, groups=0):
    n = len(a["u"])
    t = [_dev_col(a[k]) for k in F.FIELDS[scheme]]
    ok = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    ws = torch.empty(engine.rlc_workspace_bytes(n, bits), dtype=torch.uint8, device=DEV)
    arm(groups)
    accepted = getattr(engine, "verify_%s_rlc_dev" % scheme)(*t, ok, ws, window_bits=bits)
    torch.cuda.synchronize()
    return accepted, ok.cpu().numpy()


def _rejects(got, want, what):
    accepted, ok = got
    assert not accepted, "%s: a forged batch was accepted by the aggregate" % (what,)
    assert np.array_equal(ok, want), what


def _accepts(got, what):
    accepted, ok = got
    assert accepted and ok.all(), "%s: the control batch (forgery undone) was not accepted" % (what,)


# ---- verify_{single,double,vargen}_rlc_dev -------------------------------------------------------------------
DEV_CASES = [(s, kind, pair) for s in SCHEMES for kind, pair in F.unkeyed_cases(s)]


@pytest.mark.parametrize("scheme,kind,pair", DEV_CASES, ids=["%s-%s-%d-%d" % (s, k, p[0], p[1]) for s, k, p in DEV_CASES])
def test_device_form_rejects_cancelling_forgeries(engine, scheme, kind, pair):
    f, want = forged(scheme, kind, pair)
    with one_aggregate(engine) as arm:
        for bits in BITS:
            _rejects(_run_dev(engine, arm, scheme, f.forged, bits), want, bits)
            _accepts(_run_dev(engine, arm, scheme, f.honest, bits), bits)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_both_items_inside_one_forced_sub_group(engine, scheme):
    """four forced sub-groups, the pair inside sub-group 2: the other three accept, this one must not"""
    plan = engine.rlc_plan_info(scheme, N, 8, 4)
    assert plan["groups"] == 4
    pair = (2 * plan["sub"] + 4, 3 * plan["sub"] - 1)
    assert pair[1] < N
    with one_aggregate(engine) as arm:
        for kind in ("u", "R"):
            f, want = forged(scheme, kind, pair)
            _rejects(_run_dev(engine, arm, scheme, f.forged, 8, groups=4), want, kind)
            _accepts(_run_dev(engine, arm, scheme, f.honest, 8, groups=4), kind)


def _tiled(a, n, cols):
    reps = -(-n // N)
    return {k: np.ascontiguousarray(np.tile(a[k], (reps, 1))[:n]) for k in cols}


def test_pair_2_to_the_16_items_apart(engine):
    """n = 2^16 + 77, the pair (11, 11 + 2^16): a weight that depended on the low 16 bits of the item number only
    would give both the same z.  The 1543-item base tiled; the oracle ran on the base with the forged rows."""
    n = (1 << 16) + 77
    pair = (11, 11 + (1 << 16))
    rows = (pair[0] % N, pair[1] % N)
    assert rows[0] != rows[1]
    with one_aggregate(engine) as arm:
        for kind in ("u", "R"):
            f, want = forged("single", kind, rows)
            honest = _tiled(f.honest, n, F.FIELDS["single"])
            a = {k: v.copy() for k, v in honest.items()}
            expect = np.ones(n, np.uint8)
            for at, row in zip(pair, rows):
                assert not want[row]
                expect[at] = 0
                for k in a:
                    a[k][at] = f.forged[k][row]
            _rejects(_run_dev(engine, arm, "single", a, 12), expect, kind)
            _accepts(_run_dev(engine, arm, "single", honest, 12), kind)


# ---- dsv_verify_*_wire_rlc_dev -------------------------------------------------------------------------------
def _wire(scheme, a):
    cp = O.compress
    if scheme == "single":
        return np.concatenate([a["u"], cp(a["R"])], axis=1), cp(a["PK"]), a["m"]
    return (np.concatenate([a["u"], cp(a["R"]), cp(a["Rp"])], axis=1), np.concatenate([cp(a["PK"]), cp(a["PKp"])], axis=1),
            a["m"])


@pytest.mark.parametrize("scheme", ["single", "double"])
def test_wire_form_rejects_cancelling_forgeries(engine, scheme):
    """serialized records in HBM at the smallest size at which the entry point runs an aggregate by itself
    (automatic window bits): the forged pair in the first tile of the tiled base"""
    n = MIN_AUTO[scheme]
    wire_oracle = getattr(O, "verify_%s_wire" % scheme)

    def run(arm, a):
        t = [_dev_col(x) for x in _wire(scheme, a)]
        ok = torch.full((n,), 5, dtype=torch.uint8, device=DEV)
        ws = torch.empty(engine.wire_rlc_workspace_bytes(n, 0), dtype=torch.uint8, device=DEV)
        arm()
        acc = engine.verify_wire_rlc_dev(scheme, *t, ok, ws, window_bits=0)
        torch.cuda.synchronize()
        return acc, ok.cpu().numpy()

    with one_aggregate(engine) as arm:
        for kind in ("u", "R"):
            f, want = forged(scheme, kind, (5, 69))
            assert np.array_equal(wire_oracle(*_wire(scheme, f.forged)), want)
            honest = _tiled(f.honest, n, F.FIELDS[scheme])
            a = {k: v.copy() for k, v in honest.items()}
            for k in a:
                a[k][[5, 69]] = f.forged[k][[5, 69]]
            expect = np.ones(n, np.uint8)
            expect[[5, 69]] = 0
            _rejects(run(arm, a), expect, kind)
            _accepts(run(arm, honest), kind)


# ---- dsv_verify_mixed_rlc_dev --------------------------------------------------------------------------------
def test_mixed_batch_rejects_cancelling_forgeries(engine):
    """singles on even, doubles on odd positions, 2^17 of each (the singles' group just runs an aggregate): a
    u-pair inside the single kind, then — a call of its own — one cross-equation item in the double kind"""
    h = 1 << 17
    n = 2 * h
    fs, _ = forged("single", "u", (5, 69))
    fd, _ = forged("double", "cross", (5, 5))
    singles, doubles = _tiled(fs.honest, h, F.FIELDS["single"]), _tiled(fd.honest, h, F.FIELDS["double"])

    def batch(s, d):
        out = {}
        for k, w in (("u", 32), ("R", 64), ("Rp", 64), ("PK", 64), ("PKp", 64), ("m", 32)):
            t = np.zeros((n, w), np.uint8)
            if k in s:
                t[0::2] = s[k]
            t[1::2] = d[k]
            out[k] = _dev_col(t)
        return out

    kinds = (torch.arange(n, device=DEV) & 1).to(torch.uint8)
    ws = torch.empty(engine.mixed_rlc_workspace_bytes(n), dtype=torch.uint8, device=DEV)

    def run(arm, b):
        ok = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
        arm()
        acc = engine.verify_mixed_rlc_dev(kinds, b["u"], b["R"], b["Rp"], b["PK"], b["PKp"], b["m"], h, ok, ws)
        torch.cuda.synchronize()
        return acc, ok.cpu().numpy()

    with one_aggregate(engine) as arm:
        _accepts(run(arm, batch(singles, doubles)), "control")
        bad = {k: v.copy() for k, v in singles.items()}
        for k in bad:
            bad[k][[5, 69]] = fs.forged[k][[5, 69]]
        expect = np.ones(n, np.uint8)
        expect[[10, 138]] = 0
        _rejects(run(arm, batch(bad, doubles)), expect, "u-pair in the single kind")
        bad = {k: v.copy() for k, v in doubles.items()}
        for k in bad:
            bad[k][5] = fd.forged[k][5]
        expect = np.ones(n, np.uint8)
        expect[11] = 0
        _rejects(run(arm, batch(singles, bad)), expect, "cross-equation item in the double kind")


# ---- host form: typed objects, the bucket pass in two ranges -------------------------------------------------
def _limb_cols(scheme, a):
    """affine canonical columns -> the limb columns of the *_mont_cols entry points (z = 1)"""
    one = np.zeros(32, np.uint8)
    one[0] = 1
    cols = [O.to_mont(a["u"], fr=True)]
    for k in C.POINTS[scheme]:
        uvz = np.concatenate([a[k], np.tile(one, (len(a[k]), 1))], axis=1)
        cols.append(O.to_mont(np.ascontiguousarray(uvz)))
    return cols + [O.to_mont(a["m"])]


@pytest.mark.parametrize("scheme", ["single", "double"])
def test_host_form_in_two_ranges_rejects_cancelling_forgeries(engine, scheme):
    """verify_*_mont_cols_rlc from 2^18 items on: the first range's bucket pass runs while the second is on the
    bus.  Pairs (i, first + i) across the two ranges — items with the same RANGE-LOCAL number — and the two items
    at the boundary; the double scheme: one cross-equation item in the second range."""
    n = (1 << 18) + (1 << 16) + 5
    first = D.two_range_first(n, scheme != "single")
    assert n // 2 <= first < n - 256
    if scheme == "single":
        cases = [(kind, (i, first + i)) for kind in ("u", "R") for i in (0, 1, 255)]
        cases += [(kind, (first - 1, first)) for kind in ("u", "R")]
    else:
        cases = [("cross", (first + 7, first + 7))]
    honest = _tiled(F.base(scheme), n, F.FIELDS[scheme])
    views = C.as_records(scheme, _limb_cols(scheme, honest))[3]
    with one_aggregate(engine) as arm:
        arm()
        got, accepted = engine.verify_mont_cols_rlc(scheme, views)
        _accepts((accepted, got), "control")
        for kind, pair in cases:
            rows = tuple(p % N for p in pair)
            assert len(set(rows)) == len(set(pair))
            f, want = forged(scheme, kind, rows)
            limbs = _limb_cols(scheme, {k: f.forged[k][list(rows)] for k in F.FIELDS[scheme]})
            saved = [v[list(pair)].copy() for v in views]
            expect = np.ones(n, np.uint8)
            for j, at in enumerate(pair):
                assert not want[rows[j]]
                expect[at] = 0
                for v, col in zip(views, limbs):
                    v[at] = col[j]
            arm()
            got, accepted = engine.verify_mont_cols_rlc(scheme, views)
            for v, s in zip(views, saved):
                v[list(pair)] = s
            _rejects((accepted, got), expect, (kind, pair))


# ---- keyed: KeySet.verify_rlc_dev ----------------------------------------------------------------------------
KEYED_CASES = [(s, k, kind, same) for s in SCHEMES for k in F.KEY_COUNTS for kind, same in F.keyed_cases(s, k)]


@pytest.mark.parametrize("scheme,k,kind,same", KEYED_CASES,
                         ids=["%s-k%d-%s-%s" % (s, k, kd, "one" if sm else "two") for s, k, kd, sm in KEYED_CASES])
def test_keyed_form_rejects_cancelling_forgeries(engine, scheme, k, kind, same):
    """k = 1; 37 (per-workgroup key sums in LDS); 300 (beyond kKeyedLdsKeys: global atomics)"""
    f = F.forge_keyed(scheme, kind, k, (5, 69), same_key=same)
    want = F.keyed_oracle(scheme, f.forged, f.keys)
    expect = np.ones(N, np.uint8)
    expect[f.items] = 0
    assert np.array_equal(want, expect)
    P0, P1 = f.keys

    def run(arm, ks, a):
        cols = [a["u"], a["R"]] + ([a["Rp"]] if scheme == "double" else []) + [a["idx"].view(np.int32), a["m"]]
        ok = torch.full((N,), 7, dtype=torch.uint8, device=DEV)
        ws = torch.empty(engine.keyed_rlc_workspace_bytes(N, ks.k, 8), dtype=torch.uint8, device=DEV)
        arm()
        acc = ks.verify_rlc_dev(*[_dev_col(c) for c in cols], ok, ws, window_bits=8)
        torch.cuda.synchronize()
        return acc, ok.cpu().numpy()

    with one_aggregate(engine) as arm:
        with (engine.KeySet(scheme, P0, P1) if scheme != "single" else engine.KeySet(scheme, P0)) as ks:
            _rejects(run(arm, ks, f.forged), want, (k, kind, same))
            _accepts(run(arm, ks, f.honest), (k, kind, same))
