"""The storage of the lane-private joint window table (schnorr_amd/csrc/common.h: JointTable — limbs 0..7 of an
entry in a 128-byte aligned global slot, limb 8 in LDS): every verdict against the CPU oracle's, the way
tests/test_gpu_parity.py compares them.

The one-lane kernel (k_verify_fixed_half) serves batches above 2^14 items, and a device call of 2^17 items or more
is cut into 2^16-item parts, so at the library's defaults neither the small counts nor a second trip of the
grid-stride loop reach it.  The library reads DSV_QUAD / DSV_SPLIT once, at dsv_init: the last test of this file
runs the file again in a child process with both switched off, where every count below goes through the one-lane
kernel and the largest makes a lane rebuild its global and LDS slots.  (In the parent process the same tests run on
the default dispatch; the tiled batches and the open-set call reach the new layout there too.)"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import harness as H
import oracle_lib as O
import pymodel as M
import joint_model as JW

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = "DSV_TABLE_LAYOUT_CHILD"
COUNTS = (1, 63, 64, 65, 4097)
_LAUNCH_H = open(os.path.join(ROOT, "schnorr_amd", "csrc", "launch.h")).read()
GRID_CAP = int(re.search(r"kMaxVerifyGrid = (\d+);", _LAUNCH_H).group(1))
BLOCK = int(re.search(r"kVerifyBlock = (\d+);", _LAUNCH_H).group(1))
QUAD_MAX = 1 << 14

_CACHE = {}


def _batch(kind):
    """4097 signatures, every 16th corrupted (harness.tamper), and the oracle's verdicts; computed once"""
    if kind not in _CACHE:
        n = max(COUNTS)
        if kind == "single":
            d = O.keygen_sign_single(n, 2321, nthreads=8)
            H.tamper(d)
            cols = ("u", "R", "PK", "m")
            want = O.verify_single(*[d[k] for k in cols], nthreads=8)
        else:
            d = O.keygen_sign_double(n, 2322, nthreads=8)
            H.tamper(d)
            d["PKp"][5] = d["PKp"][6]      # only the primed half wrong
            d["Rp"][9] = d["Rp"][10]
            cols = ("u", "R", "Rp", "PK", "PKp", "m")
            want = O.verify_double(*[d[k] for k in cols], nthreads=8)
        want = np.asarray(want).astype(np.uint8)
        assert int(want.sum()) <= n - len(range(0, n, 16)) and want.sum() > n // 2
        _CACHE[kind] = ([np.ascontiguousarray(d[k]) for k in cols], want)
    return _CACHE[kind]


def _run_dev(engine, kind, arrays, ws_offset):
    """verdicts of verify_<kind>_dev with the workspace `ws_offset` bytes into its allocation"""
    n = len(arrays[0])
    t = [a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]
    ok = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    need = engine.workspace_bytes(n)
    ws = torch.empty(need + ws_offset, dtype=torch.uint8, device=DEV)[ws_offset:]
    assert ws.data_ptr() % 128 == ws_offset % 128 and ws.numel() == need
    (engine.verify_single_dev if kind == "single" else engine.verify_double_dev)(*t, ok, ws)
    torch.cuda.synchronize()
    return ok.cpu().numpy()


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kind", ("single", "double"))
def test_item_counts_with_an_offset_workspace(engine, kind, n):
    """n items, the workspace 16 bytes off its allocation: the table base is rounded up inside it"""
    arrays, want = _batch(kind)
    got = _run_dev(engine, kind, [a[:n] for a in arrays], 16)
    assert np.array_equal(got, want[:n]), np.flatnonzero(got != want[:n])[:8]
    if n == max(COUNTS):
        assert np.array_equal(_run_dev(engine, kind, arrays, 0), want)


def test_challenges_reach_every_digit_pair_and_both_signs():
    """what the 4097-item batch puts through the window loop, on the integer model of tests/test_joint_windows.py:
    all 16 raw digit pairs (every slot with both signs, and the identity slot) and both signs of b"""
    arrays, _ = _batch("single")
    u, R, PK, m = arrays
    c = O.challenge_single(R[:512], m[:512])
    pairs, slots, signs = set(), set(), set()
    for row in c:
        a, b, bneg = M.half_scalars(M.from_le(row))
        signs.add(bool(bneg))
        ya, yb = JW.recode_signed2(a), JW.recode_signed2(b)
        nz = (ya ^ JW.A) | (yb ^ JW.A)
        top = (nz.bit_length() - 1) >> 1 if nz else 0
        for k in range(top + 1):
            ra, rb = (ya >> (2 * k)) & 3, (yb >> (2 * k)) & 3
            pairs.add((ra, rb))
            slots.add(JW.joint_slot(ra, rb))
    assert len(pairs) == 16 and signs == {False, True}
    assert slots == {JW.joint_slot(ra, rb) for ra in range(4) for rb in range(4)}
    assert {abs(s) for s in slots} == set(range(12)) and min(slots) < 0


def _special_rows():
    """PK and R out of {(0, 1), (0, -1), an order-4 point, the item's honest value}, u out of {0, honest}: entries
    whose limbs are at their extremes (2d*t = 0, u = 0) and windows that read the identity slot"""
    sqrt_m1 = pow(7, (M.Q - 1) // 4, M.Q)
    assert M.on_curve((sqrt_m1, 0))
    pt = lambda p: np.frombuffer(M.point_bytes(p), np.uint8)
    special = [pt(M.IDENTITY), pt((0, M.Q - 1)), pt((sqrt_m1, 0))]
    d = O.keygen_sign_double(48, 5)
    rows = {k: [] for k in ("u", "R", "Rp", "PK", "PKp", "m")}
    i = 0
    for pk in range(4):
        for r in range(4):
            for zero_u in (False, True):
                rows["u"].append(np.zeros(32, np.uint8) if zero_u else d["u"][i])
                rows["R"].append(d["R"][i] if r == 3 else special[r])
                rows["PK"].append(d["PK"][i] if pk == 3 else special[pk])
                rows["Rp"].append(d["Rp"][i] if r != 1 else special[(r + pk) % 3])
                rows["PKp"].append(d["PKp"][i] if pk != 2 else special[(r + pk) % 3])
                rows["m"].append(d["m"][i])
                i += 1
    return {k: np.stack(v) for k, v in rows.items()}


def test_points_with_extreme_entries(engine):
    a = _special_rows()
    single = [a[k] for k in ("u", "R", "PK", "m")]
    double = [a[k] for k in ("u", "R", "Rp", "PK", "PKp", "m")]
    want_s = np.asarray(O.verify_single(*single)).astype(np.uint8)
    want_d = np.asarray(O.verify_double(*double)).astype(np.uint8)
    assert 2 <= want_s.sum() < len(want_s)            # 0*G + c*O == O, and the honest items
    assert np.array_equal(_run_dev(engine, "single", single, 16), want_s)
    assert np.array_equal(_run_dev(engine, "double", double, 16), want_d)
    # tiled beyond 2^14 items: the one-lane kernel whatever the dispatch switches say
    reps = QUAD_MAX // len(want_s) + 1
    tile = lambda cols: [np.tile(x, (reps, 1)) for x in cols]
    assert np.array_equal(_run_dev(engine, "single", tile(single), 16), np.tile(want_s, reps))
    assert np.array_equal(_run_dev(engine, "double", tile(double), 0), np.tile(want_d, reps))


def test_second_trip_of_the_grid_stride_loop(engine):
    """one workgroup more than the grid's cap, plus one item: unsplit (the child process), lanes 0..64 of the
    grid verify a second item and rebuild their slots.  The generator's own pattern (every 16th item corrupted) on
    all items; the oracle on both trips of those lanes and on a strided sample."""
    from schnorr_amd import workload as W
    n = GRID_CAP * BLOCK + BLOCK + 1
    b = W.gen_single(n, seed=4242)
    cols = ("u", "R", "PK", "m")
    got = _run_dev(engine, "single", [b[k] for k in cols], 16)
    want = b["expected"].cpu().numpy()
    assert n // 16 <= n - int(want.sum()) <= n // 16 + 1
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    idx = np.unique(np.concatenate([np.arange(0, BLOCK + 1), np.arange(GRID_CAP * BLOCK - 8, n),
                                    np.arange(0, n, 2741)]))
    tidx = torch.from_numpy(idx).to(DEV)
    sub = [b[k][tidx].cpu().numpy() for k in cols]
    assert np.array_equal(np.asarray(O.verify_single(*sub, nthreads=8)).astype(np.uint8), got[idx])


def test_open_set_call_with_misses(engine):
    """k_verify_listed runs the same table code: eight keys registered, every other item misses"""
    arrays, want = _batch("single")
    u, R, PK, m = arrays
    keys = np.ascontiguousarray(PK[1:9])
    known = {bytes(k) for k in keys}
    misses = sum(bytes(row) not in known for row in PK)
    with engine.KeySet("single", keys) as ks:
        assert ks.key_ok().all()
        got, nmiss = ks.verify_open(u, R, PK, m)
    assert nmiss == misses and 0 < len(PK) - misses <= 16
    assert np.array_equal(np.asarray(got).astype(np.uint8), want)


def test_one_lane_kernel_in_a_child_process(engine):
    """this file again with DSV_QUAD=0 and DSV_SPLIT=0 (read at dsv_init): see the module's docstring"""
    if os.environ.get(CHILD):
        return
    env = dict(os.environ)
    env.update({"DSV_QUAD": "0", "DSV_SPLIT": "0", CHILD: "1"})
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x",
                        "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-500:]
