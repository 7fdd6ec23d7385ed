"""The numpy model of the key census (dsv_keyset_census*, include/dsv.h) and what its suites share
(tests/test_gpu_keyset_census.py and the child process of its histogram-path test): a dict from key bytes to the
lowest valid registered index, np.unique over the missed rows, the poisoned device run with its checks, and the
cases of the model / extremes / collisions tests, built from seeds so that two processes build the same ones.
The census compares bytes only: missed keys are random bytes, registered keys come from tests/keyed_cases.py."""
import hashlib

import numpy as np

NONE = 0xFFFFFFFF
POISON32 = 0x5A5A5A5A
HITS0 = 1000  # what a hits entry holds before a call: the census adds to it


# ---- the model -----------------------------------------------------------------------------------------------
def as_rows(A, B=None):
    """the key bytes per item as one uint8 [n, w] array"""
    A = np.ascontiguousarray(A)
    return A if B is None else np.ascontiguousarray(np.hstack([A, B]))


def where_of(rows, key_ok):
    """key bytes -> the lowest index of a valid registered key"""
    d = {}
    for j in range(len(rows)):
        if key_ok[j]:
            d.setdefault(rows[j].tobytes(), j)
    return d


def model(where, rows, k, usable=None):
    """dict(idx uint32 [n], hits int64 [k], report {(rep, count)}, misses, unusable) of the items `rows` against the
    registered keys `where`; usable (optional): 0 = the item has no key bytes"""
    n = len(rows)
    usable = np.ones(n, bool) if usable is None else np.asarray(usable, bool)
    idx = np.array([where.get(rows[i].tobytes(), NONE) if usable[i] else NONE for i in range(n)], dtype=np.uint32)
    return _finish(idx, rows, k, usable)


def _finish(idx, rows, k, usable):
    hits = np.bincount(idx[idx != NONE].astype(np.int64), minlength=k)
    at = np.flatnonzero((idx == NONE) & usable)
    report = set()
    if len(at):
        _, first, counts = np.unique(rows[at], axis=0, return_index=True, return_counts=True)
        report = {(int(at[f]), int(c)) for f, c in zip(first, counts)}
    return dict(idx=idx, hits=hits, report=report, misses=int((idx == NONE).sum()), unusable=int((~usable).sum()))


def model_ids(ids, index_of_id, k):
    """the model for items given as ids into a small key population (large n): index_of_id[id] = the registered index
    of population key id, or NONE"""
    idx = np.asarray(index_of_id, dtype=np.uint32)[ids]
    hits = np.bincount(idx[idx != NONE].astype(np.int64), minlength=k)
    missed = idx == NONE
    counts = np.bincount(ids[missed], minlength=len(index_of_id))
    first = np.full(len(index_of_id), len(ids), dtype=np.int64)
    np.minimum.at(first, ids[missed], np.flatnonzero(missed))
    report = {(int(first[j]), int(counts[j])) for j in np.flatnonzero(counts)}
    return dict(idx=idx, hits=hits, report=report, misses=int(missed.sum()), unusable=0)


def sorted_report(report):
    """the host forms' order: count descending, then representative ascending -> (rep [d], count [d])"""
    r = sorted(report, key=lambda e: (-e[1], e[0]))
    return (np.array([e[0] for e in r], dtype=np.uint32), np.array([e[1] for e in r], dtype=np.uint32))


# ---- the device run ------------------------------------------------------------------------------------------
def run_dev(engine, ks, form, cols, with_idx=True, with_hits=True, hits=None, stream=None):
    """one census through KeySet.census{,_wire,_mont}_dev over host arrays `cols`, every output poisoned first ->
    dict of host arrays idx (or None), hits (or None; [capacity], HITS0 before the call unless `hits`, a device tensor,
    is given), rep, count [n], totals [4]"""
    import torch

    from keyed_cases import DEV, _dev

    n = len(cols[0])
    idx = torch.full((n,), POISON32, dtype=torch.int32, device=DEV) if with_idx else None
    if with_hits and hits is None:
        hits = torch.full((max(ks.capacity, 1),), HITS0, dtype=torch.int32, device=DEV)
    rep = torch.full((n,), POISON32, dtype=torch.int32, device=DEV)
    count = torch.full((n,), POISON32, dtype=torch.int32, device=DEV)
    totals = torch.full((4,), POISON32, dtype=torch.int32, device=DEV)
    if form == "mont":
        need = engine.keyset_census_mont_workspace_bytes(ks.scheme, n)
    else:
        need = engine.keyset_census_workspace_bytes(n)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)
    call = {"affine": ks.census_dev, "wire": ks.census_wire_dev, "mont": ks.census_mont_dev}[form]
    call(*_dev(cols), idx, hits if with_hits else None, rep, count, totals, ws, stream=stream)
    torch.cuda.synchronize()
    u32 = lambda t: None if t is None else t.cpu().numpy().view(np.uint32).copy()
    return dict(idx=u32(idx), hits=u32(hits) if with_hits else None, rep=u32(rep), count=u32(count),
                totals=u32(totals))


def check(got, want, k, what, hits_before=HITS0):
    """a device result against the model: idx, hits (added to entries below k, the rest untouched), the report as a
    set of (rep, count) with nothing written from totals[0] on, totals"""
    if got["idx"] is not None:
        bad = np.flatnonzero(got["idx"] != want["idx"])
        assert len(bad) == 0, (what, "idx", bad[:8], got["idx"][bad[:8]], want["idx"][bad[:8]])
    if got["hits"] is not None:
        before = np.broadcast_to(np.asarray(hits_before, dtype=np.int64), got["hits"].shape)
        assert (got["hits"][:k] == before[:k] + want["hits"][:k]).all(), (what, "hits", got["hits"][:k], want["hits"])
        assert (got["hits"][k:] == before[k:]).all(), (what, "hits at or beyond k were written")
    d = len(want["report"])
    assert got["totals"].tolist() == [d, want["misses"], want["unusable"], 0], (what, got["totals"], d, want["misses"])
    entries = list(zip(got["rep"][:d].tolist(), got["count"][:d].tolist()))
    assert len(set(entries)) == d and set(entries) == want["report"], (what, "report", sorted(entries)[:8],
                                                                        sorted(want["report"])[:8])
    assert (got["rep"][d:] == POISON32).all() and (got["count"][d:] == POISON32).all(), (what, "report beyond totals[0]")
    assert sum(c for _, c in entries) == want["misses"] - want["unusable"], what


def canonical(got, k):
    """what two runs of one case must agree on, as bytes: idx, hits below k, the sorted report, totals"""
    d = int(got["totals"][0])
    rep, count = sorted_report(set(zip(got["rep"][:d].tolist(), got["count"][:d].tolist())))
    parts = [got["idx"], got["hits"][:k], rep, count, got["totals"]]
    return b"".join(np.ascontiguousarray(p, dtype=np.uint32).tobytes() for p in parts)


# ---- the cases of the model, extremes and collisions tests ---------------------------------------------------
SCHEME_K = {"single": 33, "double": 47, "vargen": 70}
NS = (1, 63, 64, 65, 257, 4099)


def registered(engine, scheme, k=None, seed=0):
    """(P0, P1 or None) of k registered keys (keyed_cases._keys)"""
    from keyed_cases import _keys

    k = SCHEME_K[scheme] if k is None else k
    _, _, P0, P1 = _keys(engine, scheme, k, 7100 + 13 * k + seed)
    return np.ascontiguousarray(P0), None if P1 is None else np.ascontiguousarray(P1)


def records_of(P0, P1):
    from keyed_cases import _key_records

    return _key_records(P0, P1)


def mixed_rows(rng, reg_rows, n, pool=9):
    """n key rows: about three in four under registered keys, the rest under `pool` unregistered keys of random bytes
    with skewed use, plus a few that occur once"""
    w = reg_rows.shape[1]
    rows = reg_rows[rng.integers(0, len(reg_rows), size=n)].copy()
    strangers = rng.integers(0, 256, size=(pool, w), dtype=np.uint8)
    miss = np.flatnonzero(rng.integers(0, 4, size=n) == 0)
    rows[miss] = strangers[np.minimum(rng.integers(0, pool, size=len(miss)), rng.integers(0, pool, size=len(miss)))]
    once = miss[::7]
    rows[once] = rng.integers(0, 256, size=(len(once), w), dtype=np.uint8)
    return np.ascontiguousarray(rows)


def split(rows, scheme, form):
    """rows -> the columns a census call takes: affine (key_a[, key_b]), wire (records)"""
    if form == "affine" and scheme != "single":
        return [np.ascontiguousarray(rows[:, :64]), np.ascontiguousarray(rows[:, 64:])]
    return [rows]


def model_cases(engine):
    """case 1: (label, scheme, form, P0, P1, item rows) for every scheme, both byte forms, every n of NS"""
    out = []
    for scheme in ("single", "double", "vargen"):
        P0, P1 = registered(engine, scheme)
        for form in ("affine", "wire"):
            reg = as_rows(P0, P1) if form == "affine" else records_of(P0, P1)
            for n in NS:
                rng = np.random.default_rng(len(scheme) * 1000 + n + (form == "wire"))
                out.append(("%s/%s/n=%d" % (scheme, form, n), scheme, form, P0, P1, mixed_rows(rng, reg, n)))
    return out


def extreme_cases(engine):
    """case 2: (label, scheme, form, P0, P1, item rows); P0 = None: an empty set of capacity 4"""
    out = []
    P0, P1 = registered(engine, "single")
    reg = as_rows(P0)
    rng = np.random.default_rng(2026)
    stranger = rng.integers(0, 256, size=(1, 64), dtype=np.uint8)
    out.append(("one registered key", "single", "affine", P0, None, np.repeat(reg[5:6], 257, axis=0)))
    out.append(("one unregistered key", "single", "affine", P0, None, np.repeat(stranger, 257, axis=0)))
    # 4096 distinct misses in the 8192 slots of the call's table: its half-full limit
    out.append(("all distinct", "single", "affine", P0, None, rng.integers(0, 256, size=(4096, 64), dtype=np.uint8)))
    out.append(("empty set", "single", "affine", None, None, mixed_rows(rng, reg, 257)))
    rec = records_of(P0, None)
    out.append(("one unregistered record", "single", "wire", P0, None,
                np.repeat(rng.integers(0, 256, size=(1, 32), dtype=np.uint8), 65, axis=0)))
    out.append(("all distinct records", "single", "wire", P0, None,
                np.ascontiguousarray(np.vstack([rec[:3], rng.integers(0, 256, size=(61, 32), dtype=np.uint8)]))))
    # a two-point set with a key registered twice (3 = 7 = 20), an invalid key (5: off the curve) and items that pair
    # a registered PK with another key's second point
    D0, D1 = registered(engine, "double")
    D0, D1 = D0.copy(), D1.copy()
    for j in (7, 20):
        D0[j], D1[j] = D0[3], D1[3]
    D1[5, 40] ^= 1
    dreg = as_rows(D0, D1)
    rows = dreg[rng.integers(0, len(dreg), size=257)].copy()
    rows[::9] = dreg[7]
    rows[1::9] = dreg[5]
    rows[2::9, 64:] = dreg[11, 64:]  # (PK of some key, PK' of key 11)
    out.append(("duplicates, invalid, mixed pair", "double", "affine", D0, D1, np.ascontiguousarray(rows)))
    return out


def collision_cases(engine):
    """case 3: n = 64 items (128 slots in the call's table), missed keys found by search on the host that share a
    home slot — one group in the LAST slot, so that its walk wraps, one in another slot — at least three distinct keys
    each, with repeats, beside registered keys; for the affine and the record form of a single set"""
    out = []
    P0, _ = registered(engine, "single")
    n, cap = 64, 128
    for form, w in (("affine", 64), ("wire", 32)):
        rng = np.random.default_rng(31 + w)
        home = (lambda r: engine.keyset_home_slot("single", n, r)) if form == "affine" else \
               (lambda r: engine.keyset_wire_home_slot("single", n, r))
        groups = {cap - 1: [], 17: []}
        while any(len(g) < 4 for g in groups.values()):
            r = rng.integers(0, 256, size=w, dtype=np.uint8)
            g = groups.get(home(r))
            if g is not None and len(g) < 4:
                g.append(r)
        reg = as_rows(P0) if form == "affine" else records_of(P0, None)
        rows = reg[rng.integers(0, len(reg), size=n)].copy()
        keys = groups[cap - 1] + groups[17]
        use = (0, 0, 0, 1, 1, 2, 3, 4, 4, 4, 4, 5, 6, 6, 7)  # every key, with different counts
        for i, j in enumerate(rng.permutation(n)[:40]):
            rows[j] = keys[use[i % len(use)]]
        out.append(("collisions/%s" % form, "single", form, P0, None, np.ascontiguousarray(rows)))
    return out


def keyset_for(engine, scheme, P0, P1):
    if P0 is None:
        return engine.KeySet.reserved(scheme, 4)
    return engine.KeySet(scheme, P0, P1)


def run_case(engine, case):
    """-> (device result, model, k) of one case of the three builders above"""
    label, scheme, form, P0, P1, rows = case
    with keyset_for(engine, scheme, P0, P1) as ks:
        k = ks.k
        if k:
            reg = as_rows(P0, P1) if form == "affine" else records_of(P0, P1)
            where = where_of(reg, ks.key_ok())
        else:
            where = {}
        got = run_dev(engine, ks, form, split(rows, scheme, form))
    return got, model(where, rows, k), k


def digest(engine):
    """sha256 over the canonical outputs of every case of the three builders"""
    h = hashlib.sha256()
    for case in model_cases(engine) + extreme_cases(engine) + collision_cases(engine):
        got, want, k = run_case(engine, case)
        check(got, want, k, case[0])
        h.update(canonical(got, k))
    return h.hexdigest()
