"""The batch sizes at which the engine changes code path, read from the sources — TEST INFRASTRUCTURE.

Which kernels compute a verdict vector depends on the batch size n: the eight-lane / one-lane kernel
switch, the sub-batch split, the grid cap, the host pipeline's chunk plan, the fast accept's window bits
and its minimum group size, the two-range bucket pass...  The named constants are parsed from the
headers; thresholds written inline are pinned to the exact source text they are read from.  A change
that moves or renames one of them either moves the sizes tests/test_gpu_dispatch_edges.py runs with it
or fails tests/test_dispatch_edges.py (CPU): the matrix cannot go quietly stale.

`edges(path)` -> the sorted sizes of one entry-point path: T-1, T, T+1, T+63, T+64, T+65 for every
threshold T that applies to it, ragged sub-batch multiples, and 1, 31, 33, 255 (the eight- and
sixteen-lane workgroup shapes).
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "schnorr_amd", "csrc")

# (file, name) of every named constant the matrix follows
NAMED = (("launch.h", "kQuadMaxItems"), ("launch.h", "kVarHexMaxItems"), ("launch.h", "kMaxVerifyGrid"),
         ("launch.h", "kVerifyBlock"), ("launch.h", "kSplitThreads"), ("launch.h", "kSplitPerThread"),
         ("launch.h", "kSplitTile"), ("host_sync.h", "kSplitItems"), ("host_sync.h", "kPipeSmallCall"),
         ("rlc.h", "kRlcMinAuto"), ("rlc.h", "kRlcMaxGroup"), ("rlc.h", "kRlcTile"))
# the host pipeline's chunk defaults (host_sync.h: struct PlanParams)
PLAN_FIELDS = (("host_sync.h", "chunk"), ("host_sync.h", "first_chunk"))

# Thresholds written inline: (name, file, the exact source text, the values it holds)
PINNED = (
    ("normalize_lanes", "launch.h",
     "per_lane = n >= ((size_t)1 << 19) ? 16 : (n >= ((size_t)1 << 15) ? 8 : 1);", (1 << 15, 1 << 19)),
    ("rlc_default_bits", "rlc.h",
     "return n >= ((size_t)1 << 20) ? 16 : n >= ((size_t)1 << 17) ? 14 : n >= ((size_t)1 << 14) ? 12 : 8;",
     (1 << 14, 1 << 17, 1 << 20)),
    ("rlc_min_auto", "rlc.h",
     "inline size_t rlc_min_auto(int scheme) { return scheme == 0 ? kRlcMinAuto : (size_t)1 << 14; }", (1 << 14,)),
    ("rlc_two_ranges", "dsv_rlc.hip",
     "hook.on = staged_on && n >= ((size_t)1 << 18) && rlc_history(ctx) == 0 && force_groups <= 1;", (1 << 18,)),
    ("run_split", "dsv_host.h", "if (!ctx.split || n < 2 * kSplitItems) {", None),
    ("tables_beside_hash", "dsv_device.hip",
     "if (!(ctx.quad && ctx.small_overlap && n <= kQuadMaxItems) || t_pipeline_part) return nullptr;", None),
)

_EXPR_OK = re.compile(r"^[\w\s\*\+\-<>\(\)]+$")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _eval(expr, known):
    """a constant initialiser: integer literals, (size_t)/(unsigned) casts, <<, *, + and earlier names"""
    e = re.sub(r"\((?:size_t|unsigned|int|uint32_t)\)", "", expr).strip()
    if not _EXPR_OK.match(e):
        raise ValueError("unexpected initialiser %r" % expr)
    for name in re.findall(r"[A-Za-z_]\w*", e):
        if name not in known:
            raise ValueError("initialiser %r names %s, which is not a parsed constant" % (expr, name))
    return int(eval(e, {"__builtins__": {}}, dict(known)))  # noqa: S307 (checked above: ints and operators only)


def constants():
    """{name: value} of the named constants and the chunk defaults, parsed from the headers"""
    out = {}
    for fname, name in NAMED:
        m = re.search(r"constexpr\s+[\w:]+\s+%s\s*=\s*([^;]+);" % name, _source(fname))
        if not m:
            raise LookupError("%s: constexpr %s not found" % (fname, name))
        out[name] = _eval(m.group(1), out)
    for fname, field in PLAN_FIELDS:
        m = re.search(r"struct PlanParams\s*\{[^}]*?size_t\s+%s\s*=\s*([^;]+);" % field, _source(fname))
        if not m:
            raise LookupError("%s: PlanParams::%s not found" % (fname, field))
        out["plan_" + field] = _eval(m.group(1), out)
    return out


def pinned_missing():
    """the pinned snippets that no longer appear verbatim in their file"""
    return [(name, fname) for name, fname, text, _ in PINNED if text not in _source(fname)]


def _pinned(name):
    return next(v for n, _, _, v in PINNED if n == name)


# ---- entry-point paths ---------------------------------------------------------------------------
SCHEMES = ("single", "double", "vargen")
DEV_FORMS = ("affine", "ext", "mont", "wire")           # verify_<scheme>[_ext|_mont|_wire]_dev
HOST_FORMS = ("affine", "mont_cols", "submit", "wire")  # host memory: pageable arrays / typed objects
HOST_MAX = (1 << 18) + (1 << 16)                        # host forms stay below this (pageable copies)


def thresholds(path):
    """[(name, T)] of one path: "dev/<form>/<scheme>", "host/<form>/<scheme>", "mixed", "rlc_dev/<scheme>",
    "rlc_wire_dev/<scheme>", "rlc_host/<scheme>" (mont_cols_rlc and wire_rlc)"""
    k = constants()
    kind, _, rest = path.partition("/")
    form, _, scheme = rest.rpartition("/")
    out = []
    if kind in ("dev", "host"):
        small = k["kVarHexMaxItems"] if scheme == "vargen" else k["kQuadMaxItems"]
        out.append(("small_kernel", small))
        out.append(("grid_cap", k["kMaxVerifyGrid"] * k["kVerifyBlock"]))
        if kind == "dev":
            out.append(("run_split", 2 * k["kSplitItems"]))
            if form in ("ext", "mont"):
                out += [("normalize_lanes", t) for t in _pinned("normalize_lanes")]
        else:
            out.append(("split_items", k["kSplitItems"]))
            out.append(("pipe_small_call", k["kPipeSmallCall"]))
            out.append(("first_chunk", k["plan_first_chunk"]))
            out.append(("two_first_chunks", 2 * k["plan_first_chunk"]))
            out.append(("chunk", k["plan_chunk"]))
    elif kind == "mixed":
        out.append(("split_tile", k["kSplitTile"]))
        out.append(("small_kernel", k["kQuadMaxItems"]))
    elif kind in ("rlc_dev", "rlc_wire_dev"):
        scheme = rest
        out += [("rlc_bits", t) for t in _pinned("rlc_default_bits")]
        out.append(("rlc_min_auto", k["kRlcMinAuto"] if scheme == "single" else _pinned("rlc_min_auto")[0]))
        out.append(("grid_cap", k["kMaxVerifyGrid"] * k["kVerifyBlock"]))
    elif kind == "rlc_host":
        out.append(("rlc_min_auto", k["kRlcMinAuto"]))
        out.append(("rlc_bits", _pinned("rlc_default_bits")[1]))
        out += [("rlc_two_ranges", t) for t in _pinned("rlc_two_ranges")]
    else:
        raise ValueError("unknown path %r" % path)
    return out


def edges(path):
    """sorted batch sizes of one path (see the module docstring); host forms stay at n <= HOST_MAX"""
    k = constants()
    sizes = set()
    for _, t in thresholds(path):
        sizes.update(t + d for d in (-1, 0, 1, 63, 64, 65))
    kind = path.split("/")[0]
    if kind in ("dev", "host"):
        split = k["kSplitItems"]
        # ragged sub-batches: a one-item last part, and one that drops back into the eight-lane kernel
        sizes.update((2 * split + 1, 3 * split + k["kQuadMaxItems"] + 1))
        sizes.update((1, 31, 33, 255))
    if kind == "mixed":
        sizes.update((1, 31, 33, 255))
    if kind == "rlc_dev" and path.endswith("/single"):
        sizes.add(k["kRlcMaxGroup"] + 1)
    if kind in ("host", "rlc_host"):
        sizes = {s for s in sizes if s <= HOST_MAX}
    return sorted(s for s in sizes if s > 0)


# ---- the host pipeline's sub-batches (host_sync.h: plan_chunks / plan_parts, ramp plan) -----------
def host_parts(n, heavy=False):
    """first item of every sub-batch of a host call of n items that finds the GPU idle (the ramp plan);
    heavy: double / var-generator items.  A mirror of plan_chunks + plan_parts, used only to place
    positions: a drift makes the positions less sharp, never a test wrong."""
    k = constants()
    unit, chunk, first = k["kSplitItems"], k["plan_chunk"], k["plan_first_chunk"]
    chunks = []
    if n <= k["kPipeSmallCall"]:
        chunks = [n]
    else:
        left = staged = c = 0
        left = n
        while left:
            if heavy:
                want = unit if c < 2 else 2 * unit
            else:
                want = (first if first < unit else unit) if c < 2 else unit
                while want * 2 <= staged // 8:
                    want *= 2
            want = min(want, chunk)
            if left <= want + unit // 2 or left <= want + want // 4:
                want = left
            chunks.append(want)
            left -= want
            staged += want
            c += 1
    starts, off = [], 0
    for cnt in chunks:
        if cnt <= unit:
            part = cnt
        else:
            parts = -(-cnt // unit)
            parts += parts & 1
            part = -(-(-(-cnt // parts)) // 256) * 256
        p = 0
        while p < cnt:
            starts.append(off + p)
            p += part
        off += cnt
    return starts


def two_range_first(n, heavy=False):
    """item where the host forms' two-range bucket pass starts its second range (dsv_rlc.hip RlcHook:
    the first sub-batch at or beyond n / 2)"""
    return next(s for s in host_parts(n, heavy) if s >= n / 2 and s > 0)
