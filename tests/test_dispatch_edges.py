"""tests/dispatch_edges.py follows the sources: every named threshold is found with a plausible value,
every pinned inline threshold is still written where it was read, and edges() straddles each of them.
(CPU only: a change that moves a threshold moves the GPU matrix or fails here.)"""
import math

import pytest

import dispatch_edges as D

PATHS = ([("dev/%s/%s" % (f, s)) for f in D.DEV_FORMS for s in D.SCHEMES]
         + [("host/%s/%s" % (f, s)) for f in D.HOST_FORMS for s in D.SCHEMES]
         + ["mixed"] + ["rlc_dev/%s" % s for s in D.SCHEMES] + ["rlc_wire_dev/%s" % s for s in D.SCHEMES]
         + ["rlc_host/%s" % s for s in D.SCHEMES])


def test_named_constants_are_found_and_plausible():
    k = D.constants()
    for _, name in D.NAMED:
        assert name in k
    pow2 = lambda v: v > 0 and v & (v - 1) == 0
    for name in ("kQuadMaxItems", "kVarHexMaxItems", "kSplitItems", "kPipeSmallCall", "kRlcMinAuto", "kRlcMaxGroup",
                 "kSplitTile", "kRlcTile", "plan_chunk", "plan_first_chunk"):
        assert pow2(k[name]), (name, k[name])
    assert 1 << 10 <= k["kVarHexMaxItems"] <= k["kQuadMaxItems"] <= k["kSplitItems"] <= 1 << 20
    assert k["kVerifyBlock"] in (64, 128, 256) and 256 <= k["kMaxVerifyGrid"] <= 1 << 16
    assert k["kSplitTile"] == k["kSplitThreads"] * k["kSplitPerThread"]
    assert k["kSplitItems"] <= k["kPipeSmallCall"] * 4 and k["plan_first_chunk"] <= k["plan_chunk"] <= 1 << 22
    assert 1 << 12 <= k["kRlcMinAuto"] < k["kRlcMaxGroup"] <= 1 << 24


def test_pinned_snippets_are_still_in_their_files():
    assert D.pinned_missing() == []
    for name, fname, text, values in D.PINNED:
        for v in values or ():
            assert "<< %d)" % int(math.log2(v)) in text or "<< %d;" % int(math.log2(v)) in text, (name, v)


def test_a_reworded_snippet_is_reported(monkeypatch):
    real = D._source
    monkeypatch.setattr(D, "_source", lambda f: real(f).replace("(size_t)1 << 19", "(size_t)1 << 18"))
    assert ("normalize_lanes", "launch.h") in D.pinned_missing()


def test_a_moved_constant_moves_the_edges(monkeypatch):
    real = D._source
    before = D.edges("dev/affine/single")
    monkeypatch.setattr(D, "_source", lambda f: real(f).replace(
        "kQuadMaxItems = (size_t)1 << 14;", "kQuadMaxItems = (size_t)1 << 13;"))
    assert D.constants()["kQuadMaxItems"] == 1 << 13
    after = D.edges("dev/affine/single")
    assert (1 << 13) - 1 in after and (1 << 13) + 1 in after and (1 << 14) + 1 not in after
    assert (1 << 14) + 1 in before


@pytest.mark.parametrize("path", PATHS)
def test_edges_straddle_every_threshold(path):
    sizes = set(D.edges(path))
    limit = D.HOST_MAX if path.startswith(("host/", "rlc_host/")) else None
    assert D.thresholds(path)
    for name, t in D.thresholds(path):
        if limit and t + 1 > limit:
            continue
        assert {t - 1, t, t + 1} <= sizes, (path, name, t)
    assert min(sizes) >= 1
    if limit:
        assert max(sizes) <= limit
    if path.startswith(("dev/", "host/")):
        split = D.constants()["kSplitItems"]
        assert {1, 31, 33, 255, 2 * split + 1, 3 * split + D.constants()["kQuadMaxItems"] + 1} <= sizes


def test_the_thresholds_the_issue_lists_are_covered():
    k = D.constants()
    dev = set(D.edges("dev/ext/single"))
    assert {(1 << 15) - 1, 1 << 15, (1 << 19) + 1, (1 << 17) + 1, (1 << 18) + 1} <= dev
    assert {(1 << 13) - 1, (1 << 13) + 1} <= set(D.edges("dev/affine/vargen"))
    assert {(1 << 20) - 1, 1 << 20, (1 << 14) - 1, (1 << 14)} <= set(D.edges("rlc_dev/double"))
    assert k["kRlcMaxGroup"] + 1 in D.edges("rlc_dev/single")
    assert {(1 << 18) - 1, 1 << 18, (1 << 18) + 1, (1 << 17) - 1} <= set(D.edges("rlc_host/single"))
    assert {4095, 4096, 4097} <= set(D.edges("mixed"))


def test_host_sub_batches_cover_the_call():
    k = D.constants()
    for n in (1000, 1 << 16, (1 << 16) + 1, (1 << 18) + (1 << 14) + 3, D.HOST_MAX):
        for heavy in (False, True):
            starts = D.host_parts(n, heavy)
            assert starts[0] == 0 and starts == sorted(set(starts)) and starts[-1] < n
            gaps = [b - a for a, b in zip(starts, starts[1:] + [n])]
            assert max(gaps) <= max(k["kSplitItems"], n if n <= k["kPipeSmallCall"] else 0)
    n = (1 << 18) + (1 << 14) + 3
    assert n / 2 <= D.two_range_first(n) < n
