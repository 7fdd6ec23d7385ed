"""The key census on the GPU (dsv_keyset_census*, include/dsv.h) against the numpy model of
tests/census_model.py: per-key hit counts, the distinct missed keys with their counts and lowest items, totals, for
the affine, record and typed forms, device and host; the extremes, collisions in the call's miss table, both
histogram paths, the grid-stride loop, graph capture, and the loop closed by schnorr_amd.keycache.KeyCache."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import census_model as CM
from keyed_cases import DEV, POISON, _dev, _keys, _limbs, _poison, _scalars

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = CM.NONE
SCHEMES = ("single", "double", "vargen")


def _run_cases(engine, cases):
    for case in cases:
        got, want, k = CM.run_case(engine, case)
        CM.check(got, want, k, case[0])
    return len(cases)


# ---- 1. against the model ------------------------------------------------------------------------------------
def test_census_matches_model(engine):
    """every scheme, the affine and the record form, n in {1, 63, 64, 65, 257, 4099}: key_idx_out, hits, the report
    as a set of (rep, count), totals; every output poisoned first — the report from totals[0] on and hits from k on
    must be untouched"""
    cases = CM.model_cases(engine)
    assert _run_cases(engine, cases) == 3 * 2 * len(CM.NS)
    # the cases are what they are meant to be: hits and misses, repeated and single missed keys
    got, want, k = CM.run_case(engine, cases[len(CM.NS) - 1])
    assert 500 < want["misses"] < 1500 and len(want["report"]) > 100 and max(c for _, c in want["report"]) > 50
    assert (want["hits"] > 0).all() and k == CM.SCHEME_K["single"]


@pytest.mark.parametrize("form", ("affine", "wire"))
def test_census_without_idx_and_hits(engine, form):
    """key_idx_out and hits NULL, each alone and both: the rest of the outputs is the model's"""
    scheme = "double"
    P0, P1 = CM.registered(engine, scheme)
    reg = CM.as_rows(P0, P1) if form == "affine" else CM.records_of(P0, P1)
    rows = CM.mixed_rows(np.random.default_rng(5), reg, 257)
    with engine.KeySet(scheme, P0, P1) as ks:
        want = CM.model(CM.where_of(reg, ks.key_ok()), rows, ks.k)
        for with_idx, with_hits in ((False, True), (True, False), (False, False)):
            got = CM.run_dev(engine, ks, form, CM.split(rows, scheme, form), with_idx=with_idx, with_hits=with_hits)
            assert (got["idx"] is None) == (not with_idx) and (got["hits"] is None) == (not with_hits)
            CM.check(got, want, ks.k, (form, with_idx, with_hits))


# ---- 2. extremes ---------------------------------------------------------------------------------------------
def test_census_extremes(engine):
    cases = CM.extreme_cases(engine)
    by = {c[0]: c for c in cases}
    _run_cases(engine, cases)
    got, want, k = CM.run_case(engine, by["one registered key"])
    assert want["report"] == set() and want["hits"][5] == 257 and got["totals"].tolist() == [0, 0, 0, 0]
    got, want, k = CM.run_case(engine, by["one unregistered key"])
    assert want["report"] == {(0, 257)} and got["rep"][0] == 0 and got["count"][0] == 257
    got, want, k = CM.run_case(engine, by["all distinct"])
    assert len(want["report"]) == 4096 == want["misses"] and engine.keyset_census_workspace_bytes(4096) == 2 * 4 * 8192
    got, want, k = CM.run_case(engine, by["empty set"])
    assert k == 0 and want["misses"] == 257 and (got["idx"] == NONE).all() and (got["hits"] == CM.HITS0).all()
    got, want, k = CM.run_case(engine, by["duplicates, invalid, mixed pair"])
    # hits go to the lower index of a key registered twice; the invalid key and the mixed pairs are reported misses
    assert want["hits"][3] > 28 and want["hits"][7] == 0 == want["hits"][20] == want["hits"][5]
    rows = by["duplicates, invalid, mixed pair"][5]
    assert (1, int((rows == rows[1]).all(axis=1).sum())) in want["report"]
    assert any(rep % 9 == 2 for rep, _ in want["report"])


# ---- 3. collisions in the call's miss table -------------------------------------------------------------------
def test_census_collisions_and_wrap(engine):
    cases = CM.collision_cases(engine)
    assert _run_cases(engine, cases) == 2
    for case in cases:
        _, scheme, form, P0, _, rows = case
        home = engine.keyset_home_slot if form == "affine" else engine.keyset_wire_home_slot
        reg = {r.tobytes() for r in (CM.as_rows(P0) if form == "affine" else CM.records_of(P0, None))}
        homes = {}
        for r in {r.tobytes() for r in rows} - reg:
            homes.setdefault(home("single", 64, np.frombuffer(r, np.uint8)), []).append(r)
        assert len(homes[127]) >= 3 and len(homes[17]) >= 3, {h: len(v) for h, v in homes.items()}


# ---- 4. hits accumulate --------------------------------------------------------------------------------------
def test_hits_accumulate(engine):
    P0, _ = CM.registered(engine, "single")
    reg = CM.as_rows(P0)
    rng = np.random.default_rng(44)
    with engine.KeySet.reserved("single", 100, P0) as ks:
        assert ks.capacity == 100 and ks.k == 33
        where = CM.where_of(reg, ks.key_ok())
        hits = torch.full((100,), 5, dtype=torch.int32, device=DEV)
        total = np.full(100, 5, dtype=np.int64)
        for n in (257, 4099):
            rows = CM.mixed_rows(rng, reg, n)
            want = CM.model(where, rows, ks.k)
            got = CM.run_dev(engine, ks, "affine", [rows], hits=hits)
            CM.check(got, want, ks.k, n, hits_before=total)
            total[:ks.k] += want["hits"]
        assert (hits.cpu().numpy() == total).all() and total[:33].sum() > 3000 and (total[33:] == 5).all()


# ---- 5. both histogram paths ---------------------------------------------------------------------------------
def test_both_histogram_paths(engine):
    """DSV_CENSUS_LDS_KEYS is read at dsv_init, so the per-wave path runs in a child process: its outputs on the
    cases of tests 1 - 3 (checked against the model there too) are byte for byte this process's"""
    assert engine.census_lds_keys() == 4096
    mine = CM.digest(engine)
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from schnorr_amd import engine as E\nimport census_model as CM\nE.init(0)\n"
            "print('lds_keys', E.census_lds_keys())\nprint('digest', CM.digest(E))\n") % (ROOT, os.path.join(ROOT, "tests"))
    env = dict(os.environ, DSV_CENSUS_LDS_KEYS="0")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    out = dict(line.split() for line in r.stdout.strip().splitlines() if line.startswith(("lds_keys", "digest")))
    assert out["lds_keys"] == "0" and out["digest"] == mine, out


# ---- 6. grid-stride ------------------------------------------------------------------------------------------
def test_grid_stride(engine):
    """n = 2^20 + 257 items — more than kMaxLookupGrid * kLookupBlock = 2^20 lanes — drawn from a population of 300
    keys of which 40 are registered"""
    n, pop, k = (1 << 20) + 257, 300, 40
    P0, _ = CM.registered(engine, "single", k)
    rng = np.random.default_rng(6)
    keys = rng.integers(0, 256, size=(pop, 64), dtype=np.uint8)
    at = rng.permutation(pop)[:k]
    keys[at] = P0
    index_of = np.full(pop, NONE, dtype=np.uint32)
    index_of[at] = np.arange(k, dtype=np.uint32)
    ids = rng.integers(0, pop, size=n)
    want = CM.model_ids(ids, index_of, k)
    assert len(want["report"]) == pop - k and 800000 < want["misses"] < 1000000
    with engine.KeySet("single", P0) as ks:
        assert (ks.key_ok() == 1).all()
        got = CM.run_dev(engine, ks, "affine", [keys[ids]])
    CM.check(got, want, k, "grid-stride")


# ---- 7. the typed form ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_typed_form(engine, scheme):
    """key objects with random z: the results of the affine census over their normal form; plants with z = 0 and
    with a limb group >= q count in totals[2] and have no report entry.  Device and host form."""
    import pymodel as M

    k, extra, n = CM.SCHEME_K[scheme], 8, 257
    _, _, K0, K1 = _keys(engine, scheme, k + extra, 8800 + k)
    two = K1 is not None
    rng = np.random.default_rng(70 + k)
    j = rng.integers(0, k + extra, size=n)
    affine = [np.ascontiguousarray(K0[j])] + ([np.ascontiguousarray(K1[j])] if two else [])
    limbs = [_limbs(a, rng) for a in affine]
    usable = np.ones(n, bool)
    plants = [(3, 0, slice(64, 96), np.zeros(32, np.uint8)), (40, 0, slice(0, 32), np.full(32, 0xFF, np.uint8)),
              (41, len(limbs) - 1, slice(64, 96), np.frombuffer(M.le32(M.Q), np.uint8)),
              (200, len(limbs) - 1, slice(32, 64), np.full(32, 0xFF, np.uint8))]
    for i, col, where, value in plants:
        limbs[col][i, where] = value
        usable[i] = False
    P0 = np.ascontiguousarray(K0[:k])
    P1 = np.ascontiguousarray(K1[:k]) if two else None
    rows = CM.as_rows(*affine)
    with engine.KeySet(scheme, P0, P1) as ks:
        want = CM.model(CM.where_of(CM.as_rows(P0, P1), ks.key_ok()), rows, k, usable)
        assert want["unusable"] == 4 and 3 <= len(want["report"]) <= extra
        assert not {3, 40, 41, 200} & {r for r, _ in want["report"]}
        got = CM.run_dev(engine, ks, "mont", limbs)
        CM.check(got, want, k, (scheme, "mont dev"))
        ref = CM.run_dev(engine, ks, "affine", affine)  # the affine census over the normal form, where it is usable
        keep = usable
        assert (ref["idx"][keep] == got["idx"][keep]).all()
        host = ks.census_mont_cols(limbs)
        rep, count = CM.sorted_report(want["report"])
        assert (host["idx"] == want["idx"]).all() and (host["hits"][:k] == want["hits"]).all()
        assert (host["rep"] == rep).all() and (host["count"] == count).all()
        assert (host["misses"], host["unusable"]) == (want["misses"], 4)


# ---- 8. host forms -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ("affine", "wire"))
def test_host_forms_across_a_chunk_edge(engine, form):
    """n = 2^18 + 5: one key's items on both sides of the chunk edge — the result is the whole call's: the lowest
    item index of the call, the counts summed, sorted by count descending, then representative ascending"""
    n, chunk, scheme = (1 << 18) + 5, 1 << 18, "vargen"
    P0, P1 = CM.registered(engine, scheme)
    reg = CM.as_rows(P0, P1) if form == "affine" else CM.records_of(P0, P1)
    w, k = reg.shape[1], len(P0)
    rng = np.random.default_rng(8 + w)
    pop = np.vstack([reg, rng.integers(0, 256, size=(30, w), dtype=np.uint8)])
    ids = rng.integers(0, len(pop), size=n)
    edge, late = len(pop), len(pop) + 1  # a key on both sides of the edge, and one that only the second chunk holds
    pop = np.vstack([pop, rng.integers(0, 256, size=(2, w), dtype=np.uint8)])
    ids[[chunk - 3, chunk + 2]] = edge
    ids[chunk + 4] = late
    index_of = np.full(len(pop), NONE, dtype=np.uint32)
    index_of[:k] = np.arange(k)
    want = CM.model_ids(ids, index_of, k)
    assert (chunk - 3, 2) in want["report"] and (chunk + 4, 1) in want["report"]
    rows = np.ascontiguousarray(pop[ids])
    with engine.KeySet(scheme, P0, P1) as ks:
        assert (ks.key_ok() == 1).all()
        got = ks.census(*CM.split(rows, scheme, form)) if form == "affine" else ks.census_wire(rows)
    rep, count = CM.sorted_report(want["report"])
    assert (got["idx"] == want["idx"]).all() and (got["hits"] == want["hits"]).all()
    assert len(got["rep"]) == len(rep) == 32 and (got["rep"] == rep).all() and (got["count"] == count).all()
    assert (got["misses"], got["unusable"]) == (want["misses"], 0)


# ---- 9. capture ----------------------------------------------------------------------------------------------
def test_capture_and_replay(engine):
    """one census_dev recorded into a graph (a straight chain), replayed over inputs rewritten in place with other
    miss sets: the model's results each time, hits accumulating across the replays"""
    scheme, n = "double", 4099
    P0, P1 = CM.registered(engine, scheme)
    reg = CM.as_rows(P0, P1)
    rng = np.random.default_rng(9)
    batches = [CM.mixed_rows(rng, reg, n, pool=p) for p in (3, 9, 40)]
    with engine.KeySet(scheme, P0, P1) as ks:
        k = ks.k
        where = CM.where_of(reg, ks.key_ok())
        bufs = _dev(CM.split(batches[0], scheme, "affine"))
        new = lambda count: torch.full((count,), CM.POISON32, dtype=torch.int32, device=DEV)
        idx, rep, count, totals = new(n), new(n), new(n), new(4)
        hits = torch.zeros(k, dtype=torch.int32, device=DEV)
        ws = torch.empty(engine.keyset_census_workspace_bytes(n), dtype=torch.uint8, device=DEV)
        side = torch.cuda.Stream(device=DEV)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            ks.census_dev(*bufs, idx, hits, rep, count, totals, ws)
        torch.cuda.synchronize()
        hits.zero_()
        total = np.zeros(k, dtype=np.int64)
        for rows in batches[1:] + batches[:1]:
            for buf, a in zip(bufs, _dev(CM.split(rows, scheme, "affine"))):
                buf.copy_(a)
            for t in (idx, rep, count, totals):
                t.fill_(CM.POISON32)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            u32 = lambda t: t.cpu().numpy().view(np.uint32).copy()
            got = dict(idx=u32(idx), hits=u32(hits), rep=u32(rep), count=u32(count), totals=u32(totals))
            want = CM.model(where, rows, k)
            CM.check(got, want, k, "replay", hits_before=total)
            total += want["hits"]
        del g


# ---- 10. the loop closed -------------------------------------------------------------------------------------
def test_keycache_closes_the_loop(engine):
    """KeyCache of capacity 16 over a population of 40 signing keys: primed with a batch under 16 of the cold keys,
    then four rounds of one batch of 512 valid items with skewed use plus a few corrupted ones.  The verdicts are
    the unkeyed call's every round, the batch's misses never rise after a maintain(), and after the last one they
    are the items under keys outside the 16 most used."""
    from schnorr_amd.keycache import KeyCache

    pop, cap = 40, 16
    sk, _, P0, _ = _keys(engine, "single", pop, 10010)
    rng = np.random.default_rng(10)

    def batch(uses, corrupt):
        j = rng.permutation(np.repeat(np.arange(pop), uses))
        n = len(j)
        m, r = _scalars(rng, n, 0x3F), _scalars(rng, n, 0x07)
        u, R = engine.sign_single(sk[j], m, r)
        PK = np.ascontiguousarray(P0[j])
        for i in range(corrupt):  # wrong signatures under their own key, and key bytes nobody registered
            (u if i % 2 else PK)[7 * i + 3, 1] ^= 0x10
        return [u, R, PK, m]

    uses = np.array(list(range(35, 19, -1)) + [3] * 24)
    assert uses.sum() == 512
    args = batch(uses, 6)
    n = len(args[0])
    # the 16 most used keys, by bytes, are unambiguous
    keys, counts = np.unique(args[2], axis=0, return_counts=True)
    by_use = np.sort(counts)[::-1]
    assert by_use[cap - 1] > by_use[cap] and pop < len(keys) <= pop + 3
    outside = int(n - by_use[:cap].sum())
    assert 0 < outside < n // 4
    want = engine.verify_single(*args)
    assert 500 <= want.sum() < n
    prime = batch(np.array([0] * 16 + [8] * 16 + [0] * 8), 0)

    def run(cache, a):
        ok = _poison(len(a[0]))
        ws = torch.empty(engine.keyed_open_workspace_bytes(len(a[0])), dtype=torch.uint8, device=DEV)
        misses = torch.full((1,), 999, dtype=torch.int32, device=DEV)
        cache.verify_open_dev(*_dev(a), ok, ws, misses=misses)
        torch.cuda.synchronize()
        return ok.cpu().numpy(), int(misses.item())

    with KeyCache("single", cap) as cache:
        ok, missed = run(cache, prime)
        assert ok.all() and missed == len(prime[0])
        did = cache.maintain()
        assert did["appended"] == 16 and cache.ks.k == 16
        assert run(cache, prime)[1] == 0
        cache.maintain()
        last, replaced = None, 0
        for rnd in range(4):
            ok, missed = run(cache, args)
            assert (ok == want).all(), (rnd, np.flatnonzero(ok != want)[:8])
            assert ok[ok != POISON].size == n
            if last is not None:
                assert missed <= last, (rnd, missed, last)
            last = missed
            replaced += cache.maintain()["replaced"]
        assert replaced == 16 and cache.ks.k == cap
        ok, missed = run(cache, args)
        assert (ok == want).all() and missed == outside, (missed, outside)
