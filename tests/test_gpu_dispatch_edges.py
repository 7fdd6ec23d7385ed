"""Every batch-size dispatch boundary against the oracle (GPU).

The sizes come from tests/dispatch_edges.py, which reads them from the sources: T - 1, T, T + 1, T + 63 ..
T + 65 of every threshold a path has (kernel family, sub-batch split, grid cap, normalisation batching,
host chunk plan, fast-accept window bits, minimum group, two-range bucket pass), ragged sub-batch tails and
the small workgroup shapes.  Each case tiles a prime-length adversarial base set (tests/edge_sets.py) to n
with a size-dependent rotation, fills `ok` with a poison byte and compares the WHOLE verdict vector with the
tiled oracle vector.  The fast accept is also swept position by position: one wrong-but-well-formed item at
every sub-group edge, k_rlc_part1 tile edge, row_stride pad item and host sub-batch / two-range boundary,
which the aggregate must never accept.
"""
import numpy as np
import pytest
import torch

import dispatch_edges as D
import edge_sets as ES
import mont_cases as MC
import oracle_lib as O
from keyed_cases import _diff, _poison

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = D.constants()
POISON = 7
SUFFIX = {"affine": "", "ext": "_ext", "mont": "_mont", "wire": "_wire"}
WS = {"affine": "workspace_bytes", "ext": "ext_workspace_bytes", "mont": "mont_workspace_bytes",
      "wire": "wire_workspace_bytes"}


def _rot(n, length):
    return (n * 7919) % length


# ---- tiles of the base sets (module cache: the last few kept, device or host) -----------------------------
_TILES = {}


def _tile(scheme, form, variant, nmax, device):
    key = (scheme, form, variant, device)
    hit = _TILES.get(key)
    arrs, want = ES.base(scheme, form, variant)
    length = len(want)
    if hit is None or hit[0] < nmax:
        if len(_TILES) >= 4:
            _TILES.pop(next(iter(_TILES)))
            torch.cuda.empty_cache()
        reps = -(-(nmax + length) // length)
        if device:
            big = [torch.from_numpy(a).to(DEV).repeat(reps, 1) for a in arrs]
            w = torch.from_numpy(want).to(DEV).repeat(reps)
        else:
            big = [np.tile(a, (reps, 1)) for a in arrs]
            w = np.tile(want, reps)
        hit = _TILES[key] = (reps * length - length, big, w)
    return hit[1], hit[2], length


def _slice(scheme, form, variant, n, device=True, nmax=None):
    """(arrays, expected) of n items: the base set tiled, starting at a size-dependent rotation"""
    big, w, length = _tile(scheme, form, variant, max(n, nmax or n), device)
    r = _rot(n, length)
    return [a[r:r + n] for a in big], w[r:r + n]


def _dev_call(engine, scheme, form, arrs, n):
    ok = _poison(n)
    ws = torch.empty(getattr(engine, WS[form])(n), dtype=torch.uint8, device=DEV)
    getattr(engine, "verify_%s%s_dev" % (scheme, SUFFIX[form]))(*arrs, ok, ws)
    torch.cuda.synchronize()
    return ok


def _steady(engine):
    """the fast accept's plain plan: no sample, no sub-groups from the history, no guarded second stage"""
    engine.rlc_history(0, 0)
    engine.rlc_history_long(0, 0)


# ---- 1. per-signature entry points, device-resident -------------------------------------------------------
DEV_CASES = [(s, f, n) for s in D.SCHEMES for f in D.DEV_FORMS for n in D.edges("dev/%s/%s" % (f, s))]
DEV_MAX = {(s, f): max(D.edges("dev/%s/%s" % (f, s))) for s in D.SCHEMES for f in D.DEV_FORMS}


@pytest.mark.parametrize("scheme,form,n", DEV_CASES, ids=["%s-%s-%d" % c for c in DEV_CASES])
def test_dev_per_signature_at_every_edge(engine, scheme, form, n):
    arrs, want = _slice(scheme, form, "mixed", n, nmax=DEV_MAX[(scheme, form)])
    ok = _dev_call(engine, scheme, form, arrs, n)
    assert torch.equal(ok, want), _diff(ok, want)


def _splice_positions(path, n, block):
    """block starts straddling every threshold of the path below n, and the tail; no two overlap"""
    out = []
    for p in sorted({t - block // 2 for _, t in D.thresholds(path) if block // 2 <= t <= n - block // 2}) + [n - block]:
        if not out or p >= out[-1] + block:
            out.append(p)
    return out


@pytest.mark.parametrize("scheme,form", [(s, f) for s in D.SCHEMES for f in D.DEV_FORMS])
def test_dev_unique_blocks_across_the_boundaries(engine, scheme, form):
    """At the largest size of the path: freshly signed, distinct items spliced across every boundary and at the
    tail (tiling repeats items, so it cannot show two items aliased onto one another; these can)."""
    path = "dev/%s/%s" % (form, scheme)
    n = DEV_MAX[(scheme, form)]
    block = 256
    arrs, want = _slice(scheme, form, "mixed", n)
    arrs, want = [a.clone() for a in arrs], want.clone()
    pos = _splice_positions(path, n, block)
    f_arrs, f_want = ES.fresh(scheme, form, block * len(pos), 4200 + len(form))
    for j, p in enumerate(pos):
        for a, fa in zip(arrs, f_arrs):
            a[p:p + block] = torch.from_numpy(fa[j * block:(j + 1) * block]).to(DEV)
        want[p:p + block] = torch.from_numpy(f_want[j * block:(j + 1) * block]).to(DEV)
    ok = _dev_call(engine, scheme, form, arrs, n)
    assert torch.equal(ok, want), _diff(ok, want)


# ---- 2. per-signature entry points, host memory -----------------------------------------------------------
HOST_CASES = [(s, f, n) for s in D.SCHEMES for f in D.HOST_FORMS for n in D.edges("host/%s/%s" % (f, s))]
_RECORDS = {}


def _host_views(scheme, n):
    """column views into arrays of typed records (tests/mont_cases.py as_records), rotated like _slice"""
    if scheme not in _RECORDS:
        arrs, want = ES.base(scheme, "mont", "mixed")
        reps = -(-(D.HOST_MAX + len(want)) // len(want))
        _RECORDS.clear()
        _RECORDS[scheme] = (MC.as_records(scheme, [np.tile(a, (reps, 1)) for a in arrs])[3], np.tile(want, reps),
                            len(want))
    views, w, length = _RECORDS[scheme]
    r = _rot(n, length)
    return [v[r:r + n] for v in views], w[r:r + n]


@pytest.mark.parametrize("scheme,form,n", HOST_CASES, ids=["%s-%s-%d" % c for c in HOST_CASES])
def test_host_per_signature_at_every_edge(engine, scheme, form, n):
    if form in ("mont_cols", "submit"):
        cols, want = _host_views(scheme, n)
        if form == "mont_cols":
            got = engine.verify_mont_cols(scheme, cols)
        else:
            got = engine.submit_mont_cols(scheme, cols).wait()
    else:
        base_form = "wire" if form == "wire" else "affine"
        arrs, want = _slice(scheme, base_form, "mixed", n, device=False, nmax=D.HOST_MAX)
        got = getattr(engine, "verify_%s%s" % (scheme, "_wire" if form == "wire" else ""))(*arrs)
    assert np.array_equal(got, want), _diff(got, want)


# ---- 3. mixed batches: per-kind counts on both sides of the eight-lane switch and the split tile ----------
def _mixed_cases():
    out = []
    for t in (K["kSplitTile"], K["kQuadMaxItems"]):
        for d in (-1, 0, 1):
            out += [(t + d, 33), (33, t + d)]
    out += [(K["kQuadMaxItems"] + 1, K["kQuadMaxItems"] - 1), (K["kSplitTile"] - 1, K["kQuadMaxItems"] + 1)]
    out += [(n - n // 3, n // 3) for n in D.edges("mixed")]
    return sorted(set(out))


MIXED_CASES = _mixed_cases()


@pytest.mark.parametrize("ns,nd", MIXED_CASES, ids=["s%d-d%d" % c for c in MIXED_CASES])
def test_mixed_dev_at_every_edge(engine, ns, nd):
    n = ns + nd
    kinds = np.zeros(n, np.uint8)
    kinds[np.random.default_rng(n).permutation(n)[:nd]] = 1
    si, di = np.flatnonzero(kinds == 0), np.flatnonzero(kinds == 1)
    s_arrs, s_want = _slice("single", "affine", "mixed", max(ns, 1))
    d_arrs, d_want = _slice("double", "affine", "mixed", max(nd, 1))
    cols = {k: torch.zeros((n, 32 if k in ("u", "m") else 64), dtype=torch.uint8, device=DEV)
            for k in ES.FIELDS["double"]}
    want = torch.zeros(n, dtype=torch.uint8, device=DEV)
    si_t, di_t = torch.from_numpy(si).to(DEV), torch.from_numpy(di).to(DEV)
    for k, a in zip(ES.FIELDS["single"], s_arrs):
        cols[k][si_t] = a[:ns]
    cols["Rp"][si_t], cols["PKp"][si_t] = s_arrs[1][:ns], s_arrs[2][:ns]
    for k, a in zip(ES.FIELDS["double"], d_arrs):
        cols[k][di_t] = a[:nd]
    want[si_t], want[di_t] = s_want[:ns], d_want[:nd]
    ok = _poison(n)
    ws = torch.empty(engine.mixed_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    engine.verify_mixed_dev(torch.from_numpy(kinds).to(DEV), *[cols[k] for k in ES.FIELDS["double"]], nd, ok, ws)
    torch.cuda.synchronize()
    assert torch.equal(ok, want), _diff(ok, want)


# ---- 4. the batch fast accept at its boundaries -----------------------------------------------------------
def _min_auto(scheme, host):
    return K["kRlcMinAuto"] if host or scheme == "single" else D._pinned("rlc_min_auto")[0]


def _rlc_dev_call(engine, scheme, form, arrs, n, bits=0):
    ok = _poison(n)
    if form == "wire":
        ws = torch.empty(engine.wire_rlc_workspace_bytes(n, bits), dtype=torch.uint8, device=DEV)
        accepted = engine.verify_wire_rlc_dev(scheme, *arrs, ok, ws, window_bits=bits)
    else:
        ws = torch.empty(engine.rlc_workspace_bytes(n, bits), dtype=torch.uint8, device=DEV)
        accepted = getattr(engine, "verify_%s_rlc_dev" % scheme)(*arrs, ok, ws, window_bits=bits)
    torch.cuda.synchronize()
    return accepted, ok


RLC_DEV_CASES = ([(s, "affine", n) for s in D.SCHEMES for n in D.edges("rlc_dev/%s" % s)]
                 + [(s, "wire", n) for s in D.SCHEMES for n in D.edges("rlc_wire_dev/%s" % s)])


@pytest.mark.parametrize("scheme,form,n", RLC_DEV_CASES, ids=["%s-%s-%d" % c for c in RLC_DEV_CASES])
def test_rlc_dev_accepts_clean_and_rejects_mixed_at_every_edge(engine, scheme, form, n):
    """clean tile: accepted exactly when an aggregate runs (automatic bits: n >= rlc_min_auto); mixed tile:
    never accepted; both: the whole verdict vector is the oracle's"""
    nmax = max(D.edges("rlc_%sdev/%s" % ("wire_" if form == "wire" else "", scheme)))
    for variant in ("clean", "mixed"):
        arrs, want = _slice(scheme, form, variant, n, nmax=nmax)
        _steady(engine)
        accepted, ok = _rlc_dev_call(engine, scheme, form, arrs, n)
        assert torch.equal(ok, want), (variant, _diff(ok, want))
        assert accepted == (variant == "clean" and n >= _min_auto(scheme, False)), variant
    _steady(engine)


RLC_HOST_CASES = [(s, f, n) for s in D.SCHEMES for f in ("mont_cols", "wire") for n in D.edges("rlc_host/%s" % s)]


def _host_rlc_call(engine, scheme, form, arrs):
    if form == "mont_cols":
        return engine.verify_mont_cols_rlc(scheme, arrs)
    return engine.verify_wire_rlc(scheme, *arrs)


def _host_rlc_arrays(scheme, form, variant, n):
    if form == "mont_cols":
        arrs, want = _slice(scheme, "mont", variant, n, device=False, nmax=D.HOST_MAX)
        return MC.as_records(scheme, [np.ascontiguousarray(a) for a in arrs])[3], want
    return _slice(scheme, "wire", variant, n, device=False, nmax=D.HOST_MAX)


@pytest.mark.parametrize("scheme,form,n", RLC_HOST_CASES, ids=["%s-%s-%d" % c for c in RLC_HOST_CASES])
def test_rlc_host_accepts_clean_and_rejects_mixed_at_every_edge(engine, scheme, form, n):
    for variant in ("clean", "mixed"):
        arrs, want = _host_rlc_arrays(scheme, form, variant, n)
        _steady(engine)
        ok, accepted = _host_rlc_call(engine, scheme, form, arrs)
        assert np.array_equal(ok, want), (variant, _diff(ok, want))
        assert accepted == (variant == "clean" and K["kRlcMinAuto"] <= n <= K["kRlcMaxGroup"]), variant
    _steady(engine)


# ---- 5. positional single-defect sweep of the fast accept -------------------------------------------------
# defects: (array index, byte slice) per form — every input the aggregate consumes separately
def _defects(scheme, form):
    if form == "wire":
        sig = [("u", 0, slice(0, 32)), ("R", 0, slice(32, 64))] + ([("Rp", 0, slice(64, 96))] if scheme == "double" else [])
        pk = [("PK", 1, slice(0, 32))] + ([("PKp" if scheme == "double" else "Gen", 1, slice(32, 64))]
                                           if scheme != "single" else [])
        return sig + pk + [("m", 2, slice(0, 32))]
    return [(f, j, slice(None)) for j, f in enumerate(ES.FIELDS[scheme])]


def _group_positions(n, sub, pad_from=True):
    """per sub-group: its first two items, its last, the items at multiples of kRlcTile (+-1) inside it, the
    items of the row_stride pad (the last sz mod 8)"""
    out = []
    for s in range(0, n, sub):
        sz = min(sub, n - s)
        p = {s, s + 1, s + sz - 1}
        for t in range(K["kRlcTile"], sz, K["kRlcTile"]):
            p.update((s + t - 1, s + t, s + t + 1))
        p.update(range(s + sz - sz % 8, s + sz))
        out.append(sorted(x for x in p if s <= x < s + sz))
    return out


def _oracle_form(scheme, form, arrs):
    if form == "affine":
        return getattr(O, "verify_" + scheme)(*arrs, nthreads=8)
    if form == "wire":
        return getattr(O, "verify_%s_wire" % scheme)(*arrs)
    return getattr(O, "verify_%s_mont" % scheme)(*arrs)


class _Sweep:
    """one call's victims on a clean tile: victim i takes the fields of an honest item a (so its defect is the
    only one), then field f of another honest item b — well-formed, just wrong"""

    def __init__(self, scheme, form, arrs, want):
        self.scheme, self.form, self.arrs = scheme, form, arrs
        w = want.cpu().numpy() if isinstance(want, torch.Tensor) else want
        self.want = w
        self.honest = np.flatnonzero(w == 1)
        self.defects = _defects(scheme, form)

    def plant(self, victims, k):
        """-> (saved rows, expected verdicts)"""
        saved = [(i, [a[i].clone() if isinstance(a, torch.Tensor) else a[i].copy() for a in self.arrs]) for i in victims]
        rows = []
        for j, i in enumerate(victims):
            a_i = int(self.honest[(i * 31 + 7) % len(self.honest)])
            b_i = int(self.honest[(i * 31 + 7 + 97 * (j + 1)) % len(self.honest)])
            name, arr, sl = self.defects[(k + j) % len(self.defects)]
            for x in self.arrs:
                x[i] = x[a_i]
            self.arrs[arr][i, sl] = self.arrs[arr][b_i, sl]
            rows.append(i)
        # the victims are wrong by the oracle (and the donors' rows are what they were)
        got = _oracle_form(self.scheme, self.form, [np.ascontiguousarray(
            (a.cpu().numpy() if isinstance(a, torch.Tensor) else a)[rows]) for a in self.arrs])
        assert not got.any(), (victims, got)
        expect = self.want.copy()
        expect[rows] = 0
        return saved, expect

    def restore(self, saved):
        for i, rows in saved:
            for a, r in zip(self.arrs, rows):
                a[i] = r


SWEEP_DEV = [("single", "affine", 100003, 8, 1), ("single", "affine", 100003, 12, 2),
             ("single", "affine", 100003, 8, 7), ("single", "affine", 100003, 12, 16),
             ("single", "affine", (1 << 17) + (1 << 14) + 3, 0, 1), ("single", "affine", (1 << 17) + (1 << 14) + 3, 0, 2),
             ("double", "affine", 40009, 0, 1), ("double", "affine", 40009, 8, 7),
             ("vargen", "affine", 40009, 0, 2), ("vargen", "affine", 40009, 12, 16),
             ("single", "wire", 100003, 8, 7), ("double", "wire", 40009, 0, 16)]


@pytest.mark.parametrize("scheme,form,n,bits,groups", SWEEP_DEV, ids=["%s-%s-%d-c%d-g%d" % c for c in SWEEP_DEV])
def test_rlc_dev_single_defect_sweep(engine, scheme, form, n, bits, groups):
    """one wrong item per sub-group per call, at every sub-group edge, tile edge and pad item: never accepted,
    and the verdicts are the clean tile's with exactly the victims cleared"""
    plan = engine.rlc_plan_info(scheme, n, bits, groups)
    assert (plan["groups"] > 1) == (groups > 1), plan
    arrs, want = _slice(scheme, form, "clean", n)
    arrs = [a.clone() for a in arrs]
    sw = _Sweep(scheme, form, arrs, want)
    per_group = _group_positions(n, plan["sub"])
    prev = engine.rlc_subgroups(groups)
    try:
        for k in range(max(len(p) for p in per_group)):
            victims = [p[k] for p in per_group if k < len(p)]
            saved, expect = sw.plant(victims, k)
            _steady(engine)
            accepted, ok = _rlc_dev_call(engine, scheme, form, arrs, n, bits)
            sw.restore(saved)
            assert not accepted, victims
            assert np.array_equal(ok.cpu().numpy(), expect), (victims, _diff(ok, expect))
    finally:
        engine.rlc_subgroups(prev)
        _steady(engine)


SWEEP_HOST = [("single", "mont_cols"), ("double", "mont_cols"), ("single", "wire"), ("vargen", "wire")]


@pytest.mark.parametrize("scheme,form", SWEEP_HOST)
def test_rlc_host_two_range_single_defect_sweep(engine, scheme, form):
    """the host forms' two-range bucket pass (n >= 2^18): one wrong item at first - 1 / first of the second
    range, at every host sub-batch boundary (+-1), the tail and the row_stride pad"""
    n = (1 << 18) + (1 << 14) + 3
    heavy = scheme != "single"
    first = D.two_range_first(n, heavy)
    pos = {first - 1, first, first + 1, 0, 1, n - 1}
    for s in D.host_parts(n, heavy):
        pos.update((s - 1, s, s + 1))
    pos.update(range(n - n % 8, n))
    pos = sorted(p for p in pos if 0 <= p < n)
    arrs, want = _host_rlc_arrays(scheme, form, "clean", n)
    if form == "wire":
        arrs = [a.copy() for a in arrs]
    sw = _Sweep(scheme, "mont" if form == "mont_cols" else form, arrs, want)
    _steady(engine)
    ok, accepted = _host_rlc_call(engine, scheme, form, arrs)
    assert accepted and np.array_equal(ok, want)
    try:
        for k, p in enumerate(pos):
            saved, expect = sw.plant([p], k)
            _steady(engine)
            ok, accepted = _host_rlc_call(engine, scheme, form, arrs)
            sw.restore(saved)
            assert not accepted, p
            assert np.array_equal(ok, expect), (p, _diff(ok, expect))
    finally:
        _steady(engine)
