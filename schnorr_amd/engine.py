"""Batch entry points of the MI355X engine over numpy (host buffers) and torch (HBM-resident)
arrays.  Thin marshalling only — all arithmetic happens in libdsv.so's HIP kernels.

Array conventions (see include/dsv.h): uint8, C-contiguous,
  scalars  [n, 32]   points [n, 64] (affine u || v)   ext points [n, 96] (u || v || z)
Returns uint8 verdict vectors [n] (1 = the reference's verify() would return true).
"""
import ctypes

import numpy as np

from . import _lib

_initialised = set()


def init(device=0):
    """dsv_init: create the context of one GPU (fixed-base tables, streams).  Idempotent; several
    devices may be initialised in one process."""
    if device in _initialised:
        return
    L = _lib.load()
    _lib.check(L.dsv_init(device))
    _initialised.add(device)


def init_visible():
    """dsv_init_visible: every device listed in $DSV_DEVICES, else every visible one; returns the
    list of initialised ordinals."""
    rc = _lib.load().dsv_init_visible()
    if rc < 0:
        _lib.check(rc)
    devs = initialized_devices()
    _initialised.update(devs)
    return devs


def set_device(device):
    """Device of this thread's host-buffer entry points (default: the first one initialised)."""
    _lib.check(_lib.load().dsv_set_device(device))


def initialized_devices():
    buf = (ctypes.c_int * 16)()
    n = _lib.load().dsv_initialized_devices(buf, 16)
    return [buf[i] for i in range(min(n, 16))]


def device_numa(device=0):
    """dsv_device_numa: {"bdf": PCI address, "node": NUMA node of the device's PCIe root (-1: unknown or
    DSV_NUMA=0), "cpus": that node's cpus} — where the device's copy threads are bound"""
    cpus = (ctypes.c_int * 1024)()
    node = ctypes.c_int(-1)
    bdf = ctypes.create_string_buffer(32)
    n = _lib.load().dsv_device_numa(device, ctypes.byref(node), cpus, 1024, bdf)
    if n < 0:
        _lib.check(n)
    return {"bdf": bdf.value.decode(), "node": node.value, "cpus": [cpus[i] for i in range(min(n, 1024))]}


def numa_lookup(sysfs_root, bdf):
    """dsv_debug_numa_lookup: (node, cpus) of a PCI device under a sysfs tree; no device needed"""
    cpus = (ctypes.c_int * 4096)()
    node = ctypes.c_int(-1)
    n = _lib.load().dsv_debug_numa_lookup(sysfs_root.encode(), bdf.encode(), ctypes.byref(node), cpus, 4096)
    if n < 0:
        _lib.check(n)
    return node.value, [cpus[i] for i in range(min(n, 4096))]


def shutdown(device=None):
    """dsv_shutdown (all devices) or dsv_shutdown_device."""
    if not _initialised:
        return
    if device is None:
        _lib.check(_lib.load().dsv_shutdown())
        _initialised.clear()
    else:
        _lib.check(_lib.load().dsv_shutdown_device(device))
        _initialised.discard(device)


def set_host_threads(n):
    """Copy threads of the host entry points (0 = default); returns the value in force."""
    return int(_lib.load().dsv_set_host_threads(n))


def version():
    return _lib.load().dsv_version().decode()


def _arr(a, width):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim == 1 and a.shape[0] == width:
        a = a.reshape(1, width)
    if a.ndim != 2 or a.shape[1] != width:
        raise ValueError("expected uint8 array of shape [n, %d], got %r" % (width, a.shape))
    return a


def _p(a):
    return a.ctypes.data


def _same_n(*arrs):
    n = arrs[0].shape[0]
    for a in arrs:
        if a.shape[0] != n:
            raise ValueError("batch arrays disagree on n: %r" % [x.shape for x in arrs])
    return n


# Per scheme: the fields of an item (u, the points in the canonical order, m) and the wire record widths
# (signature, public key).  Point widths by form: affine 64 B, projective / Montgomery limbs 96 B.
_SCHEMES = {"single": (("u", "R", "PK", "m"), (64, 32)),
            "double": (("u", "R", "Rp", "PK", "PKp", "m"), (96, 64)),
            "vargen": (("u", "R", "PK", "Gen", "m"), (64, 64))}
_SCHEME_CODE = {"single": 0, "double": 1, "vargen": 2}  # the C ABI's scheme argument
_KEY_POINTS = {"single": 1, "double": 2, "vargen": 2}  # points of a key: PK / PK, PK' / PK, Gen
_POINT_WIDTH = {"": 64, "_ext": 96, "_mont": 96}


def _layout(scheme, form):
    """(names, widths) of one call's arrays: form "", "_ext", "_mont" (an item's fields) or "_wire" (records)"""
    if form == "_wire":
        sw, pw = _SCHEMES[scheme][1]
        return ("sig", "pk", "m"), (sw, pw, 32)
    fields = _SCHEMES[scheme][0]
    pw = _POINT_WIDTH[form]
    names = tuple(f if f in ("u", "m") or not form else f + "_uvz" for f in fields)
    return names, tuple(32 if f in ("u", "m") else pw for f in fields)


# ------------------------------------------------------------------ host-buffer path
def _host(scheme, form, arrays, multi=False, rlc=False):
    """dsv_verify_<scheme><form>[_multi | _rlc] over host arrays -> verdicts (rlc: (verdicts, accepted))"""
    _, widths = _layout(scheme, form)
    arrs = [_arr(a, w) for a, w in zip(arrays, widths)]
    n = _same_n(*arrs)
    ok = np.zeros(n, dtype=np.uint8)
    name = "dsv_verify_%s%s%s" % (scheme, form, "_multi" if multi else "_rlc" if rlc else "")
    accepted = ctypes.c_int(0)
    tail = [ctypes.byref(accepted)] if rlc else []
    _lib.check(getattr(_lib.load(), name)(*([_p(a) for a in arrs] + [n, _p(ok)] + tail)))
    return (ok, bool(accepted.value)) if rlc else ok


def verify_single(u, R, PK, m):
    return _host("single", "", (u, R, PK, m))


def verify_double(u, R, Rp, PK, PKp, m):
    return _host("double", "", (u, R, Rp, PK, PKp, m))


def verify_vargen(u, R, PK, Gen, m):
    return _host("vargen", "", (u, R, PK, Gen, m))


def verify_single_multi(u, R, PK, m):
    """dsv_verify_single_multi: one host batch sharded over every initialised device."""
    return _host("single", "", (u, R, PK, m), multi=True)


def verify_double_multi(u, R, Rp, PK, PKp, m):
    return _host("double", "", (u, R, Rp, PK, PKp, m), multi=True)


def verify_vargen_multi(u, R, PK, Gen, m):
    return _host("vargen", "", (u, R, PK, Gen, m), multi=True)


def to_hash_inputs(uvz):
    """JubJubExtended::to_hash_inputs over [n, 96] (u || v || z) -> ([n, 64] affine, ok[n])."""
    uvz = _arr(uvz, 96)
    n = uvz.shape[0]
    out = np.zeros((n, 64), dtype=np.uint8)
    ok = np.zeros(n, dtype=np.uint8)
    _lib.check(_lib.load().dsv_to_hash_inputs(_p(uvz), n, _p(out), _p(ok)))
    return out, ok


def verify_single_ext(u, R_uvz, PK_uvz, m, multi=False):
    """Projective points (u || v || z, 96 B): the device does to_hash_inputs."""
    return _host("single", "_ext", (u, R_uvz, PK_uvz, m), multi)


def verify_double_ext(u, R_uvz, Rp_uvz, PK_uvz, PKp_uvz, m, multi=False):
    return _host("double", "_ext", (u, R_uvz, Rp_uvz, PK_uvz, PKp_uvz, m), multi)


def verify_vargen_ext(u, R_uvz, PK_uvz, Gen_uvz, m, multi=False):
    return _host("vargen", "_ext", (u, R_uvz, PK_uvz, Gen_uvz, m), multi)


# ---- the reference's in-memory representation: every element = four u64 Montgomery limbs (R = 2^256)
def verify_single_mont(u, R_uvz, PK_uvz, m, multi=False):
    return _host("single", "_mont", (u, R_uvz, PK_uvz, m), multi)


def verify_double_mont(u, R_uvz, Rp_uvz, PK_uvz, PKp_uvz, m, multi=False):
    return _host("double", "_mont", (u, R_uvz, Rp_uvz, PK_uvz, PKp_uvz, m), multi)


def verify_vargen_mont(u, R_uvz, PK_uvz, Gen_uvz, m, multi=False):
    return _host("vargen", "_mont", (u, R_uvz, PK_uvz, Gen_uvz, m), multi)


def _columns(scheme, cols):
    """(n, dsv_column array) of typed-object columns: one uint8 [n, width] array per field, rows strided,
    bytes of a row contiguous"""
    _, widths = _layout(scheme, "_mont")
    if len(cols) != len(widths):
        raise ValueError("dsv_verify_%s_mont_cols takes %d columns" % (scheme, len(widths)))
    n = cols[0].shape[0]
    arr = (_lib.Column * len(cols))()
    for k, (c, w) in enumerate(zip(cols, widths)):
        if c.dtype != np.uint8 or c.ndim != 2 or c.shape != (n, w) or (w > 1 and c.strides[1] != 1) \
                or c.strides[0] < w:
            raise ValueError("column %d: expected uint8 [n, %d] rows with contiguous bytes, got %r / strides %r"
                             % (k, w, c.shape, c.strides))
        arr[k].base = c.ctypes.data
        arr[k].stride = c.strides[0]
    return n, arr


def verify_mont_cols(scheme, cols):
    """dsv_verify_*_mont_cols: the fields of typed objects where they lie.  cols: one uint8 array
    [n, width] per field in the scheme's column order (single: u, R, PK, m; double: u, R, R', PK, PK',
    m; vargen: u, R, PK, Gen, m) — typically VIEWS into arrays of records (numpy structured arrays,
    `records["R"][:, :96]`): only the last axis has to be contiguous, the row stride is passed on."""
    n, arr = _columns(scheme, cols)
    ok = np.zeros(n, dtype=np.uint8)
    _lib.check(getattr(_lib.load(), "dsv_verify_%s_mont_cols" % scheme)(arr, n, _p(ok)))
    return ok


def verify_mont_cols_rlc(scheme, cols):
    """dsv_verify_*_mont_cols_rlc: the same columns through the batch fast accept -> (verdicts, accepted)"""
    n, arr = _columns(scheme, cols)
    ok = np.zeros(n, dtype=np.uint8)
    accepted = ctypes.c_int(0)
    _lib.check(getattr(_lib.load(), "dsv_verify_%s_mont_cols_rlc" % scheme)(arr, n, _p(ok),
                                                                          ctypes.byref(accepted)))
    return ok, bool(accepted.value)


class MontColsJob:
    """A batch in flight (dsv_verify_*_mont_cols_submit): `wait()` blocks until the verdicts are
    there and returns them.  Keeps the column arrays alive until then."""

    def __init__(self, scheme, cols):
        n, arr = _columns(scheme, cols)
        self._cols = cols
        self._ok = np.zeros(n, dtype=np.uint8)
        self._job = ctypes.c_void_p()
        _lib.check(getattr(_lib.load(), "dsv_verify_%s_mont_cols_submit" % scheme)(
            arr, n, _p(self._ok), ctypes.byref(self._job)))

    def __del__(self):
        # a job dropped unwaited still reads the columns and writes the verdicts: wait before they go
        try:
            if getattr(self, "_job", None) is not None and self._job.value is not None:
                self.wait()
        except Exception:  # noqa: BLE001
            pass

    def done(self):
        return self._job.value is None or _lib.load().dsv_job_done(self._job) == 1

    def wait(self):
        if self._job.value is not None:
            job, self._job = self._job, ctypes.c_void_p()
            _lib.check(_lib.load().dsv_job_wait(job))
            self._cols = None
        return self._ok


def submit_mont_cols(scheme, cols):
    """Asynchronous verify_mont_cols: returns a MontColsJob at once; up to max_in_flight() batches
    per device overlap (the second one's ramp runs under the first one's tail)."""
    return MontColsJob(scheme, cols)


def max_in_flight():
    return int(_lib.load().dsv_max_in_flight())


def challenge_single(R, m):
    R, m = _arr(R, 64), _arr(m, 32)
    n = _same_n(R, m)
    c = np.zeros((n, 32), dtype=np.uint8)
    _lib.check(_lib.load().dsv_challenge_single(_p(R), _p(m), n, _p(c)))
    return c


def challenge_double(R, Rp, m):
    R, Rp, m = _arr(R, 64), _arr(Rp, 64), _arr(m, 32)
    n = _same_n(R, Rp, m)
    c = np.zeros((n, 32), dtype=np.uint8)
    _lib.check(_lib.load().dsv_challenge_double(_p(R), _p(Rp), _p(m), n, _p(c)))
    return c


def sign_single(sk, m, r):
    sk, m, r = _arr(sk, 32), _arr(m, 32), _arr(r, 32)
    n = _same_n(sk, m, r)
    u = np.zeros((n, 32), dtype=np.uint8)
    R = np.zeros((n, 64), dtype=np.uint8)
    _lib.check(_lib.load().dsv_sign_single(_p(sk), _p(m), _p(r), n, _p(u), _p(R)))
    return u, R


def sign_double(sk, m, r):
    sk, m, r = _arr(sk, 32), _arr(m, 32), _arr(r, 32)
    n = _same_n(sk, m, r)
    u = np.zeros((n, 32), dtype=np.uint8)
    R = np.zeros((n, 64), dtype=np.uint8)
    Rp = np.zeros((n, 64), dtype=np.uint8)
    _lib.check(_lib.load().dsv_sign_double(_p(sk), _p(m), _p(r), n, _p(u), _p(R), _p(Rp)))
    return u, R, Rp


def sign_vargen(sk, Gen, m, r):
    sk, Gen, m, r = _arr(sk, 32), _arr(Gen, 64), _arr(m, 32), _arr(r, 32)
    n = _same_n(sk, Gen, m, r)
    u = np.zeros((n, 32), dtype=np.uint8)
    R = np.zeros((n, 64), dtype=np.uint8)
    _lib.check(_lib.load().dsv_sign_vargen(_p(sk), _p(Gen), _p(m), _p(r), n, _p(u), _p(R)))
    return u, R


def public_keys(sk, which=0, Gen=None):
    sk = _arr(sk, 32)
    n = sk.shape[0]
    PK = np.zeros((n, 64), dtype=np.uint8)
    g = None
    if Gen is not None:
        g = _arr(Gen, 64)
        _same_n(sk, g)
    _lib.check(_lib.load().dsv_public_keys(_p(sk), which, _p(g) if g is not None else None, n, _p(PK)))
    return PK


def decompress_points(comp):
    """JubJubAffine::from_bytes over [n, 32] compressed points -> ([n, 64] affine, ok[n])."""
    comp = _arr(comp, 32)
    n = comp.shape[0]
    out = np.zeros((n, 64), dtype=np.uint8)
    ok = np.zeros(n, dtype=np.uint8)
    _lib.check(_lib.load().dsv_decompress_points(_p(comp), n, _p(out), _p(ok)))
    return out, ok


def compress_points(uv):
    """JubJubAffine::to_bytes: v with bit 255 = lowest bit of u (pure byte shuffling)."""
    uv = _arr(uv, 64)
    out = np.zeros((uv.shape[0], 32), dtype=np.uint8)
    _lib.check(_lib.load().dsv_compress_points(_p(uv), uv.shape[0], _p(out)))
    return out


def verify_single_wire(sig64, pk32, m):
    return _host("single", "_wire", (sig64, pk32, m))


def verify_wire_rlc(scheme, sig, pk, m):
    """dsv_verify_*_wire_rlc: serialized records in host memory through the batch fast accept ->
    (verdicts, accepted)"""
    return _host(scheme, "_wire", (sig, pk, m), rlc=True)


def verify_double_wire(sig96, pk64, m):
    return _host("double", "_wire", (sig96, pk64, m))


def verify_vargen_wire(sig64, pk64, m):
    return _host("vargen", "_wire", (sig64, pk64, m))


def stdrng_sign_inputs(seed, n, first_item=0):
    """(sk, m, nonce) of items first_item.. of the reference harness's StdRng(seed) stream."""
    sk = np.zeros((n, 32), dtype=np.uint8)
    m = np.zeros((n, 32), dtype=np.uint8)
    r = np.zeros((n, 32), dtype=np.uint8)
    _lib.check(_lib.load().dsv_stdrng_sign_inputs(seed, first_item, n, _p(sk), _p(m), _p(r)))
    return sk, m, r


def stdrng_sign_inputs_dev(seed, sk, m, r, first_item=0, stream=None):
    n, dev = _rows((sk, 32, "sk"), (m, 32, "m"), (r, 32, "r"))
    _lib.check(_lib.load().dsv_stdrng_sign_inputs_dev(
        seed, first_item, n, _tp(sk, 32), _tp(m, 32), _tp(r, 32), _stream_ptr(stream, dev)))


def debug_table_entry(which, window, digit):
    out = np.zeros(96, dtype=np.uint8)
    _lib.check(_lib.load().dsv_debug_table_entry(which, window, digit, _p(out)))
    return out


def fixed_window_bits():
    return int(_lib.load().dsv_fixed_window_bits())


def debug_lattice3(u, c):
    """(x, y, z) the var-generator kernel uses for (u, c), as Python integers per item."""
    u, c = _arr(u, 32), _arr(c, 32)
    n = _same_n(u, c)
    out = np.zeros((n, 128), dtype=np.uint8)
    _lib.check(_lib.load().dsv_debug_lattice3(_p(u), _p(c), n, _p(out)))
    res = []
    for row in out:
        v = [int.from_bytes(row[32 * k:32 * k + 32].tobytes(), "little") for k in range(3)]
        res.append(tuple(-v[k] if row[96 + k] else v[k] for k in range(3)))
    return res


def debug_half_scalars(c):
    """(a, b) the fixed-generator kernels use for c (a >= 0, b signed), as Python integers per item."""
    c = _arr(c, 32)
    n = c.shape[0]
    out = np.zeros((n, 96), dtype=np.uint8)
    _lib.check(_lib.load().dsv_debug_half_scalars(_p(c), n, _p(out)))
    res = []
    for row in out:
        a, b = (int.from_bytes(row[32 * k:32 * k + 32].tobytes(), "little") for k in range(2))
        res.append((a, -b if row[64] else b))
    return res


def debug_fq_mul(a, b):
    a, b = _arr(a, 32), _arr(b, 32)
    n = _same_n(a, b)
    out = np.zeros((n, 32), dtype=np.uint8)
    _lib.check(_lib.load().dsv_debug_fq_mul(_p(a), _p(b), n, _p(out)))
    return out


# ------------------------------------------------------------------ HBM-resident path (torch)
# Every wrapper checks what the C ABI cannot: dtype, device, contiguity, row width, that all
# arrays of a call have the same number of rows and live on one GPU, and that verdict / workspace
# buffers are large enough — a mismatched caller gets a ValueError, not an out-of-bounds kernel.
def _t(t, width=None, name="tensor"):
    import torch

    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous()):
        raise ValueError("%s: expected a contiguous CUDA tensor" % name)
    if width is not None:
        if t.dtype != torch.uint8 or t.dim() != 2 or t.shape[1] != width:
            raise ValueError("%s: expected uint8 [n, %d], got %s %r" % (name, width, t.dtype, tuple(t.shape)))
    return t


def _rows(*named):
    """named: (tensor, width, name) triples -> n; all on one device, all with n rows"""
    n = named[0][0].shape[0]
    dev = named[0][0].device
    for t, w, name in named:
        _t(t, w, name)
        if t.shape[0] != n:
            raise ValueError("batch arrays disagree on n: %s has %d rows, expected %d" % (name, t.shape[0], n))
        if t.device != dev:
            raise ValueError("%s is on %s, the rest of the batch on %s" % (name, t.device, dev))
    return n, dev


def _bytes_out(t, need, dev, name):
    import torch

    _t(t, None, name)
    if t.dtype != torch.uint8 or t.numel() < need:
        raise ValueError("%s: need a uint8 CUDA tensor of >= %d elements, got %s x %d"
                         % (name, need, t.dtype, t.numel()))
    if t.device != dev:
        raise ValueError("%s is on %s, the batch on %s" % (name, t.device, dev))
    return t.data_ptr()


def _tp(t, width):
    return _t(t, width).data_ptr()


def workspace_bytes(n):
    return int(_lib.load().dsv_workspace_bytes(n))


def mixed_workspace_bytes(n):
    return int(_lib.load().dsv_mixed_workspace_bytes(n))


def split_scratch_bytes(n):
    return int(_lib.load().dsv_split_scratch_bytes(n))


def ext_workspace_bytes(n):
    return int(_lib.load().dsv_ext_workspace_bytes(n))


def wire_workspace_bytes(n):
    return int(_lib.load().dsv_wire_workspace_bytes(n))


def _stream_ptr(stream, dev=None):
    import torch

    s = stream if stream is not None else torch.cuda.current_stream(dev)
    return s.cuda_stream


def _dev(scheme, form, arrays, ok, workspace, stream, rlc=None):
    """dsv_verify_<scheme><form>_dev (rlc = (window_bits, accepted_out): ..._rlc_dev) over CUDA tensors.
    Returns what the fast accept decided when the call waits for it (see _accepted_arg), else None."""
    names, widths = _layout(scheme, form)
    n, dev = _rows(*zip(arrays, widths, names))
    if rlc is not None:
        window_bits, accepted_out = rlc
        arg, box = _accepted_arg(accepted_out, dev)
        ws_need = (wire_rlc_workspace_bytes if form == "_wire" else rlc_workspace_bytes)(n, window_bits)
        tail, name = [window_bits, arg], "dsv_verify_%s%s_rlc_dev" % (scheme, form)
    else:
        box = None
        ws_need = {"": workspace_bytes, "_ext": ext_workspace_bytes, "_mont": mont_workspace_bytes,
                   "_wire": wire_workspace_bytes}[form](n)
        tail, name = [], "dsv_verify_%s%s_dev" % (scheme, form)
    _lib.check(getattr(_lib.load(), name)(
        *[_tp(t, w) for t, w in zip(arrays, widths)], n, _bytes_out(ok, n, dev, "ok"),
        _bytes_out(workspace, ws_need, dev, "workspace"), _stream_ptr(stream, dev), *tail))
    return bool(box.value) if box is not None else None


def verify_single_dev(u, R, PK, m, ok, workspace, stream=None):
    """Enqueue on `stream` (default: torch's current stream of the batch's device); does not
    synchronise."""
    _dev("single", "", (u, R, PK, m), ok, workspace, stream)


def rlc_workspace_bytes(n, window_bits=0):
    b = int(_lib.load().dsv_rlc_workspace_bytes(n, window_bits))
    if b == 0:
        raise ValueError("window_bits must be 0 or one of 4, 6, 8, 12, 14, 16")
    return b


# out[24] of dsv_rlc_plan_info / dsv_keyed_rlc_plan_info
_PLAN_FIELDS = ("c", "half", "wpk", "wr", "windows", "nseg", "nseg2", "fine_bits", "kmul", "lpts", "spts", "fixed",
                "entries", "buckets", "tmp0", "tmp1", "coarse_bits", "rows", "row_stride", "bins", "bin_cap", "groups",
                "sub", "bytes")


def _plan(fn, scheme, *args):
    """fn(scheme code, *args, out[24]) -> dict of _PLAN_FIELDS"""
    out = (ctypes.c_uint64 * 24)()
    _lib.check(fn(_SCHEME_CODE[scheme], *args, out))
    return dict(zip(_PLAN_FIELDS, [int(x) for x in out]))


def _history(fn, device, set_to):
    """a dsv_debug_*history* counter: its value before the call; set_to >= 0 overrides it"""
    r = fn(device, set_to)
    if r < 0:
        _lib.check(r)
    return r


def rlc_plan_info(scheme, n, window_bits=0, groups=1):
    """dsv_rlc_plan_info as a dict (no GPU needed)"""
    return _plan(_lib.load().dsv_rlc_plan_info, scheme, n, window_bits, groups)


def rlc_history(device=0, set_to=-1):
    """dsv_debug_rlc_history: the device's fast-accept history counter (> 0: the next call checks a sample
    and runs in sub-groups); set_to >= 0 overrides it.  Returns the value before the call."""
    return _history(_lib.load().dsv_debug_rlc_history, device, set_to)


def rlc_history_long(device=0, set_to=-1):
    """dsv_debug_rlc_history_long: the slow counter behind "guarded" calls; returns the value before the call"""
    return _history(_lib.load().dsv_debug_rlc_history_long, device, set_to)


def rlc_subgroups(groups=-1):
    """dsv_debug_rlc_subgroups: force `groups` sub-groups per group (0: automatic); returns the previous setting"""
    return int(_lib.load().dsv_debug_rlc_subgroups(groups))


def _accepted_arg(accepted_out, dev):
    """the `accepted` argument of the *_rlc_dev calls: None -> a host int (the call waits for the stream and
    returns a bool); a one-element int32 tensor on `dev` or in pinned host memory -> written by the device
    when the stream gets there, the call does not block and returns None"""
    if accepted_out is None:
        box = ctypes.c_int(0)
        return ctypes.byref(box), box
    import torch

    t = accepted_out
    if t.dtype != torch.int32 or t.numel() < 1 or not (t.is_cuda and t.device == dev or (not t.is_cuda and t.is_pinned())):
        raise ValueError("accepted_out: need an int32 tensor on the batch's device or in pinned host memory")
    return t.data_ptr(), None


def verify_single_rlc_dev(u, R, PK, m, ok, workspace, stream=None, window_bits=0, accepted_out=None):
    """dsv_verify_single_rlc_dev: the verdict vector of verify_single_dev, through one aggregate test
    per group (or sub-group) when it is valid.  Enqueue-only when `accepted_out` (an int32 tensor on the
    device or in pinned host memory) is given: it receives 1 if every group was accepted by its aggregates
    once the stream gets there.  Without it the call waits for `stream` and returns that as a bool.  Never inside
    a graph capture (refused: the weights are drawn per call; so are the wire and mixed forms)."""
    return _dev("single", "", (u, R, PK, m), ok, workspace, stream, (window_bits, accepted_out))


def verify_double_rlc_dev(u, R, Rp, PK, PKp, m, ok, workspace, stream=None, window_bits=0, accepted_out=None):
    return _dev("double", "", (u, R, Rp, PK, PKp, m), ok, workspace, stream, (window_bits, accepted_out))


def verify_vargen_rlc_dev(u, R, PK, Gen, m, ok, workspace, stream=None, window_bits=0, accepted_out=None):
    return _dev("vargen", "", (u, R, PK, Gen, m), ok, workspace, stream, (window_bits, accepted_out))


def verify_double_dev(u, R, Rp, PK, PKp, m, ok, workspace, stream=None):
    _dev("double", "", (u, R, Rp, PK, PKp, m), ok, workspace, stream)


def verify_vargen_dev(u, R, PK, Gen, m, ok, workspace, stream=None):
    _dev("vargen", "", (u, R, PK, Gen, m), ok, workspace, stream)


def verify_single_ext_dev(u, R_uvz, PK_uvz, m, ok, workspace, stream=None):
    _dev("single", "_ext", (u, R_uvz, PK_uvz, m), ok, workspace, stream)


def verify_double_ext_dev(u, R_uvz, Rp_uvz, PK_uvz, PKp_uvz, m, ok, workspace, stream=None):
    _dev("double", "_ext", (u, R_uvz, Rp_uvz, PK_uvz, PKp_uvz, m), ok, workspace, stream)


def verify_vargen_ext_dev(u, R_uvz, PK_uvz, Gen_uvz, m, ok, workspace, stream=None):
    _dev("vargen", "_ext", (u, R_uvz, PK_uvz, Gen_uvz, m), ok, workspace, stream)


def mont_workspace_bytes(n):
    return int(_lib.load().dsv_mont_workspace_bytes(n))


def verify_single_mont_dev(u, R_uvz, PK_uvz, m, ok, workspace, stream=None):
    """Montgomery limbs (the Rust types' in-memory form) resident in HBM."""
    _dev("single", "_mont", (u, R_uvz, PK_uvz, m), ok, workspace, stream)


def verify_double_mont_dev(u, R_uvz, Rp_uvz, PK_uvz, PKp_uvz, m, ok, workspace, stream=None):
    _dev("double", "_mont", (u, R_uvz, Rp_uvz, PK_uvz, PKp_uvz, m), ok, workspace, stream)


def verify_vargen_mont_dev(u, R_uvz, PK_uvz, Gen_uvz, m, ok, workspace, stream=None):
    _dev("vargen", "_mont", (u, R_uvz, PK_uvz, Gen_uvz, m), ok, workspace, stream)


def verify_single_wire_dev(sig64, pk32, m, ok, workspace, stream=None):
    """Serialized records resident in HBM: Signature (64 B) / PublicKey (32 B) per item."""
    _dev("single", "_wire", (sig64, pk32, m), ok, workspace, stream)


def verify_double_wire_dev(sig96, pk64, m, ok, workspace, stream=None):
    _dev("double", "_wire", (sig96, pk64, m), ok, workspace, stream)


def verify_vargen_wire_dev(sig64, pk64, m, ok, workspace, stream=None):
    _dev("vargen", "_wire", (sig64, pk64, m), ok, workspace, stream)


def wire_rlc_workspace_bytes(n, window_bits=0):
    b = int(_lib.load().dsv_wire_rlc_workspace_bytes(n, window_bits))
    if b == 0:
        raise ValueError("window_bits must be 0 or one of 4, 6, 8, 12, 14, 16")
    return b


def verify_wire_rlc_dev(scheme, sig, pk, m, ok, workspace, stream=None, window_bits=0):
    """dsv_verify_*_wire_rlc_dev: serialized records resident in HBM through the batch fast accept.
    Blocks on `stream`; returns True if the aggregate decided every group."""
    return _dev(scheme, "_wire", (sig, pk, m), ok, workspace, stream, (window_bits, None))


def verify_core_dev(u, c, valid, PK, R, ok, workspace, which=0, accumulate=False, stream=None):
    n, dev = _rows((u, 32, "u"), (c, 32, "c"), (PK, 64, "PK"), (R, 64, "R"))
    _lib.check(_lib.load().dsv_verify_core_dev(
        _tp(u, 32), _tp(c, 32), _bytes_out(valid, n, dev, "valid"), _tp(PK, 64), _tp(R, 64),
        which, 1 if accumulate else 0, n,
        _bytes_out(ok, n, dev, "ok"), _bytes_out(workspace, workspace_bytes(n), dev, "workspace"),
        _stream_ptr(stream, dev)))


def verify_core_double_dev(u, c, valid, PK, R, PKp, Rp, ok, workspace, stream=None):
    n, dev = _rows((u, 32, "u"), (c, 32, "c"), (PK, 64, "PK"), (R, 64, "R"), (PKp, 64, "PKp"),
                   (Rp, 64, "Rp"))
    _lib.check(_lib.load().dsv_verify_core_double_dev(
        _tp(u, 32), _tp(c, 32), _bytes_out(valid, n, dev, "valid"), _tp(PK, 64), _tp(R, 64),
        _tp(PKp, 64), _tp(Rp, 64), n, _bytes_out(ok, n, dev, "ok"),
        _bytes_out(workspace, workspace_bytes(n), dev, "workspace"), _stream_ptr(stream, dev)))


def verify_mixed_dev(kinds, u, R, Rp, PK, PKp, m, n_double, ok, workspace, stream=None):
    """dsv_verify_mixed_dev: kinds uint8 [n] (0 single, 1 double), SoA over all n items."""
    n, dev = _rows((u, 32, "u"), (R, 64, "R"), (Rp, 64, "Rp"), (PK, 64, "PK"), (PKp, 64, "PKp"),
                   (m, 32, "m"))
    _lib.check(_lib.load().dsv_verify_mixed_dev(
        _bytes_out(kinds, n, dev, "kinds"), _tp(u, 32), _tp(R, 64), _tp(Rp, 64), _tp(PK, 64),
        _tp(PKp, 64), _tp(m, 32), n, int(n_double),
        _bytes_out(ok, n, dev, "ok"), _bytes_out(workspace, mixed_workspace_bytes(n), dev, "workspace"),
        _stream_ptr(stream, dev)))


def mixed_rlc_workspace_bytes(n):
    return int(_lib.load().dsv_mixed_rlc_workspace_bytes(n))


def verify_mixed_rlc_dev(kinds, u, R, Rp, PK, PKp, m, n_double, ok, workspace, stream=None):
    """dsv_verify_mixed_rlc_dev: the mixed batch with each kind through the batch fast accept; waits for
    `stream` (a host int receives the verdict); returns True if every group of both kinds was decided by its
    aggregates."""
    n, dev = _rows((u, 32, "u"), (R, 64, "R"), (Rp, 64, "Rp"), (PK, 64, "PK"), (PKp, 64, "PKp"),
                   (m, 32, "m"))
    accepted = ctypes.c_int(0)
    _lib.check(_lib.load().dsv_verify_mixed_rlc_dev(
        _bytes_out(kinds, n, dev, "kinds"), _tp(u, 32), _tp(R, 64), _tp(Rp, 64), _tp(PK, 64),
        _tp(PKp, 64), _tp(m, 32), n, int(n_double),
        _bytes_out(ok, n, dev, "ok"), _bytes_out(workspace, mixed_rlc_workspace_bytes(n), dev, "workspace"),
        _stream_ptr(stream, dev), ctypes.byref(accepted)))
    return bool(accepted.value)


def _idx(t, need, dev, name):
    import torch

    _t(t, None, name)
    if t.dtype not in (torch.int32, torch.uint32) or t.numel() < need or t.device != dev:
        raise ValueError("%s: need a 32-bit index tensor of >= %d elements on %s" % (name, need, dev))
    return t.data_ptr()


def _col32(t, n, dev, name):
    """an index or output column of a _dev form: a 32-bit tensor of shape [n] on `dev` -> its address"""
    p = _idx(t, n, dev, name)
    if t.dim() != 1 or t.shape[0] != n:
        raise ValueError("%s: expected [n] = [%d], got %r" % (name, n, tuple(t.shape)))
    return p


def split_kinds_dev(kinds, idx_single, idx_double, scratch, stream=None):
    """Stable split of the index vector by kind; returns nothing — the two counts are the last two
    int32 of `scratch` (view: scratch[-256:-248].view(torch.int32))."""
    n = kinds.numel()
    dev = kinds.device
    _lib.check(_lib.load().dsv_split_kinds_dev(
        _bytes_out(kinds, n, dev, "kinds"), n,
        _idx(idx_single, 0, dev, "idx_single"), idx_single.numel(),
        _idx(idx_double, 0, dev, "idx_double"), idx_double.numel(),
        _bytes_out(scratch, split_scratch_bytes(n), dev, "scratch"), _stream_ptr(stream, dev)))


def split_counts(scratch):
    """The two device-side counts (int32 [2] view: kind 0, kind 1) the last split left in `scratch`."""
    import torch

    return scratch[-256:-248].view(torch.int32)


def _limit_ptr(limit, dev):
    import torch

    if limit is None:
        return None
    if not (isinstance(limit, torch.Tensor) and limit.is_cuda and limit.device == dev
            and limit.dtype in (torch.int32, torch.uint32) and limit.numel() >= 1):
        raise ValueError("limit: need a 32-bit CUDA tensor of one element on %s" % dev)
    return limit.data_ptr()


def gather_rows_dev(src, idx, count, dst, limit=None, stream=None):
    """dst[j] = src[idx[j]] for j < min(count, limit[0]); src/dst uint8 [*, row_bytes], row_bytes %
    16 == 0.  `limit`: one-element 32-bit device tensor (e.g. split_counts(scratch)[k:k+1]) —
    entries of idx beyond it are never read; an index >= src.shape[0] is skipped."""
    _t(src, src.shape[1], "src")
    _t(dst, src.shape[1], "dst")
    dev = src.device
    if dst.shape[0] < count or dst.device != dev:
        raise ValueError("dst too small or on another device")
    _lib.check(_lib.load().dsv_gather_rows_dev(
        src.data_ptr(), src.shape[0], src.shape[1], _idx(idx, count, dev, "idx"), count, _limit_ptr(limit, dev),
        dst.data_ptr(), _stream_ptr(stream, dev)))


def scatter_verdicts_dev(src, idx, count, dst, limit=None, stream=None):
    """dst[idx[j]] = src[j] for j < min(count, limit[0]) (uint8 verdicts back into batch order); an
    index >= dst.numel() is skipped."""
    dev = dst.device
    _lib.check(_lib.load().dsv_scatter_verdicts_dev(
        _bytes_out(src, count, dev, "src"), _idx(idx, count, dev, "idx"), count,
        _limit_ptr(limit, dev), _bytes_out(dst, 0, dev, "dst"), dst.numel(),
        _stream_ptr(stream, dev)))


def challenge_double_dev(R, Rp, m, c, valid=None, stream=None):
    n, dev = _rows((R, 64, "R"), (Rp, 64, "Rp"), (m, 32, "m"), (c, 32, "c"))
    _lib.check(_lib.load().dsv_challenge_double_dev(
        _tp(R, 64), _tp(Rp, 64), _tp(m, 32), n, _tp(c, 32),
        _bytes_out(valid, n, dev, "valid") if valid is not None else None,
        _stream_ptr(stream, dev)))


def challenge_single_dev(R, m, c, valid=None, stream=None):
    n, dev = _rows((R, 64, "R"), (m, 32, "m"), (c, 32, "c"))
    _lib.check(_lib.load().dsv_challenge_single_dev(
        _tp(R, 64), _tp(m, 32), n, _tp(c, 32),
        _bytes_out(valid, n, dev, "valid") if valid is not None else None,
        _stream_ptr(stream, dev)))


def decompress_points_dev(comp, out_uv, ok, in_stride=32, accumulate=False, stream=None):
    """comp: uint8 CUDA tensor holding one 32-byte record every in_stride bytes."""
    n = out_uv.shape[0]
    dev = out_uv.device
    _t(comp, None, "comp")
    if comp.numel() * comp.element_size() < (n - 1) * in_stride + 32 or comp.device != dev:
        raise ValueError("comp holds fewer than n records of stride %d (or is on another device)" % in_stride)
    _lib.check(_lib.load().dsv_decompress_points_dev(
        comp.data_ptr(), in_stride, n, _tp(out_uv, 64), _bytes_out(ok, n, dev, "ok"), 1 if accumulate else 0,
        _stream_ptr(stream, dev)))


def sign_single_dev(sk, m, r, u, R, stream=None):
    n, dev = _rows((sk, 32, "sk"), (m, 32, "m"), (r, 32, "r"), (u, 32, "u"), (R, 64, "R"))
    _lib.check(_lib.load().dsv_sign_single_dev(
        _tp(sk, 32), _tp(m, 32), _tp(r, 32), n, _tp(u, 32), _tp(R, 64),
        _stream_ptr(stream, dev)))


def sign_double_dev(sk, m, r, u, R, Rp, stream=None):
    n, dev = _rows((sk, 32, "sk"), (m, 32, "m"), (r, 32, "r"), (u, 32, "u"), (R, 64, "R"), (Rp, 64, "Rp"))
    _lib.check(_lib.load().dsv_sign_double_dev(
        _tp(sk, 32), _tp(m, 32), _tp(r, 32), n, _tp(u, 32), _tp(R, 64),
        _tp(Rp, 64), _stream_ptr(stream, dev)))


def public_keys_dev(sk, which, PK, stream=None):
    n, dev = _rows((sk, 32, "sk"), (PK, 64, "PK"))
    _lib.check(_lib.load().dsv_public_keys_dev(
        _tp(sk, 32), which, n, _tp(PK, 64), _stream_ptr(stream, dev)))


def public_keys_vargen_dev(sk, Gen, PK, workspace, stream=None):
    n, dev = _rows((sk, 32, "sk"), (Gen, 64, "Gen"), (PK, 64, "PK"))
    _lib.check(_lib.load().dsv_public_keys_vargen_dev(
        _tp(sk, 32), _tp(Gen, 64), n, _tp(PK, 64),
        _bytes_out(workspace, workspace_bytes(n), dev, "workspace"), _stream_ptr(stream, dev)))


def sign_vargen_dev(sk, Gen, m, r, u, R, workspace, stream=None):
    n, dev = _rows((sk, 32, "sk"), (Gen, 64, "Gen"), (m, 32, "m"), (r, 32, "r"), (u, 32, "u"),
                   (R, 64, "R"))
    _lib.check(_lib.load().dsv_sign_vargen_dev(
        _tp(sk, 32), _tp(Gen, 64), _tp(m, 32), _tp(r, 32), n, _tp(u, 32),
        _tp(R, 64), _bytes_out(workspace, workspace_bytes(n), dev, "workspace"),
        _stream_ptr(stream, dev)))


def stdrng_vargen_inputs_dev(seed, sk, g, m, r, first_item=0, stream=None):
    n, dev = _rows((sk, 32, "sk"), (g, 32, "g"), (m, 32, "m"), (r, 32, "r"))
    _lib.check(_lib.load().dsv_stdrng_vargen_inputs_dev(
        seed, first_item, n, _tp(sk, 32), _tp(g, 32), _tp(m, 32), _tp(r, 32), _stream_ptr(stream, dev)))


# ------------------------------------------------------------------ registered key sets
def _code(scheme):
    """the C ABI's scheme argument"""
    if scheme not in _SCHEME_CODE:
        raise ValueError("scheme must be one of %s" % sorted(_SCHEME_CODE))
    return _SCHEME_CODE[scheme]


def _slots(ptrs, slots=2):
    """the pointers of a scheme's columns in an argument list with `slots` places for them: the rest are null"""
    ptrs = list(ptrs)
    return ptrs + [None] * (slots - len(ptrs))


def keyset_bytes(scheme, k):
    """dsv_keyset_bytes: device bytes of a key set of k keys (no GPU needed)"""
    return int(_lib.load().dsv_keyset_bytes(_SCHEME_CODE[scheme], k))


def keyed_workspace_bytes(n):
    return int(_lib.load().dsv_keyed_workspace_bytes(n))


def keyed_wire_workspace_bytes(scheme, n):
    """dsv_keyed_wire_workspace_bytes: device bytes of KeySet.verify_wire_dev's workspace (no GPU needed)"""
    return int(_lib.load().dsv_keyed_wire_workspace_bytes(_code(scheme), n))


def keyed_mont_workspace_bytes(scheme, n):
    """dsv_keyed_mont_workspace_bytes: device bytes of KeySet.verify_mont_dev's workspace (no GPU needed)"""
    return int(_lib.load().dsv_keyed_mont_workspace_bytes(_code(scheme), n))


def keyset_index_bytes(scheme, k):
    """dsv_keyset_index_bytes: device bytes of the index over a key set's own keys (KeySet.lookup; no GPU needed);
    not part of keyset_bytes"""
    return int(_lib.load().dsv_keyset_index_bytes(_code(scheme), k))


def keyed_lookup_workspace_bytes(n):
    """dsv_keyed_lookup_workspace_bytes: device bytes of KeySet.verify_lookup_dev's workspace (no GPU needed)"""
    return int(_lib.load().dsv_keyed_lookup_workspace_bytes(n))


def keyed_open_workspace_bytes(n):
    """dsv_keyed_open_workspace_bytes: device bytes of KeySet.verify_open_dev's workspace (no GPU needed)"""
    return int(_lib.load().dsv_keyed_open_workspace_bytes(n))


def keyset_wire_index_bytes(scheme, k):
    """dsv_keyset_wire_index_bytes: device bytes of the index over the compressed records of a key set's own keys
    (KeySet.lookup_wire; no GPU needed); not part of keyset_bytes or keyset_index_bytes"""
    return int(_lib.load().dsv_keyset_wire_index_bytes(_code(scheme), k))


def keyed_open_wire_workspace_bytes(scheme, n):
    """dsv_keyed_open_wire_workspace_bytes: device bytes of KeySet.verify_open_wire_dev's workspace (no GPU needed)"""
    return int(_lib.load().dsv_keyed_open_wire_workspace_bytes(_code(scheme), n))


def keyed_open_mont_workspace_bytes(scheme, n):
    """dsv_keyed_open_mont_workspace_bytes: device bytes of KeySet.verify_open_mont_dev's workspace (no GPU needed)"""
    return int(_lib.load().dsv_keyed_open_mont_workspace_bytes(_code(scheme), n))


def keyset_census_workspace_bytes(n):
    """dsv_keyset_census_workspace_bytes: device bytes of KeySet.census_dev's / census_wire_dev's workspace — the
    call's miss table (no GPU needed)"""
    return int(_lib.load().dsv_keyset_census_workspace_bytes(n))


def keyset_census_mont_workspace_bytes(scheme, n):
    """dsv_keyset_census_mont_workspace_bytes: device bytes of KeySet.census_mont_dev's workspace (no GPU needed)"""
    return int(_lib.load().dsv_keyset_census_mont_workspace_bytes(_code(scheme), n))


def census_lds_keys():
    """dsv_debug_census_lds_keys: up to how many keys a set's hits are counted per workgroup in LDS, as this process
    runs it (DSV_CENSUS_LDS_KEYS, read by init)"""
    return int(_lib.load().dsv_debug_census_lds_keys())


def keyset_wire_home_slot(scheme, capacity, record):
    """dsv_debug_keyset_wire_home_slot: where the probe for a key record (32 bytes per key point) starts in the
    wire index of a set of `capacity` keys (no GPU needed)"""
    code = _code(scheme)
    rec = _arr(record, _SCHEMES[scheme][1][1])
    if rec.shape[0] != 1:
        raise ValueError("one key record at a time")
    slot = ctypes.c_uint64()
    _lib.check(_lib.load().dsv_debug_keyset_wire_home_slot(code, capacity, _p(rec), ctypes.byref(slot)))
    return int(slot.value)


KEY_NONE = 0xFFFFFFFF  # DSV_KEY_NONE: the index of a key that is not in the set


def keyset_home_slot(scheme, k, key_a, key_b=None):
    """dsv_debug_keyset_home_slot: where the probe for a key (64 bytes per point) starts in the index of a set of
    k keys (no GPU needed)"""
    code = _code(scheme)
    if k < 1:
        raise ValueError("k must be at least 1")
    if (key_b is None) != (scheme == "single"):
        raise ValueError("scheme %s takes %s" % (scheme, "key_a only" if scheme == "single" else "key_a and key_b"))
    keys = [_arr(key, 64) for key in (key_a, key_b) if key is not None]
    if any(key.shape[0] != 1 for key in keys):
        raise ValueError("one key at a time")
    return int(_lib.load().dsv_debug_keyset_home_slot(code, k, *_slots(_p(key) for key in keys)))


def keyset_slots(ks, form):
    """dsv_debug_keyset_slots: the slot array of one of a KeySet's indices — form 0 / "affine": over the affine
    bytes, 1 / "record": over the compressed records — as uint32 [slots]; a slot holds a key index or KEY_NONE"""
    form = {"affine": 0, "record": 1}.get(form, form)
    L = _lib.load()
    slots = ctypes.c_size_t()
    _lib.check(L.dsv_debug_keyset_slots(ks._handle(), form, None, 0, ctypes.byref(slots)))
    out = np.zeros(slots.value, dtype=np.uint32)
    _lib.check(L.dsv_debug_keyset_slots(ks._handle(), form, _p(out), out.shape[0], ctypes.byref(slots)))
    return out


def _keyed_mont_widths(scheme):
    """widths of a keyed typed batch's columns: u, R[, R'], key_idx, m"""
    return [32] + [96] * (2 if scheme == "double" else 1) + [4, 32]


def _keyed_columns(cols, widths, what):
    """(n, dsv_column array, the arrays) of strided uint8 [n, width] views — rows strided by the object size,
    bytes of a row contiguous; a 4-byte column (key_idx) may also be a uint32 [n] array or strided view.  The
    arrays are returned so that the caller keeps them alive"""
    if len(cols) != len(widths):
        raise ValueError("%s takes %d columns" % (what, len(widths)))
    held = [np.asarray(c) for c in cols]
    n = held[0].shape[0]
    arr = (_lib.Column * len(held))()
    for k, (c, w) in enumerate(zip(held, widths)):
        as_u32 = w == 4 and c.dtype == np.uint32 and c.shape == (n,)
        # an empty array has no rows to lay out, and numpy reports its strides as it pleases (0 in recent versions)
        as_rows = c.dtype == np.uint8 and c.shape == (n, w) and (n == 0 or w == 1 or c.strides[1] == 1)
        if not (as_u32 or as_rows) or (n > 1 and c.strides[0] < w):
            raise ValueError("column %d: expected uint8 [n, %d] rows with contiguous bytes%s, got %s %r / strides %r"
                             % (k, w, " or uint32 [n]" if w == 4 else "", c.dtype, c.shape, c.strides))
        arr[k].base = c.ctypes.data
        arr[k].stride = c.strides[0] if n > 1 else max(c.strides[0], w)
    return n, arr, held


class KeyedMontColsJob(MontColsJob):
    """A keyed typed batch in flight (dsv_verify_keyed_mont_cols_submit): MontColsJob's interface.  Keeps the
    key set and the column arrays alive until the wait."""
    _symbol, _what, _widths = "dsv_verify_keyed_mont_cols_submit", "submit_mont_cols", staticmethod(_keyed_mont_widths)

    def __init__(self, keyset, cols):  # noqa: D107 (does not call the base constructor: another entry point)
        n, arr, held = _keyed_columns(cols, self._widths(keyset.scheme), self._what)
        self._cols = (keyset, held)
        self._ok = np.zeros(n, dtype=np.uint8)
        self._job = ctypes.c_void_p()
        _lib.check(getattr(_lib.load(), self._symbol)(keyset._handle(), arr, n, _p(self._ok), ctypes.byref(self._job)))


class KeyedOpenMontColsJob(KeyedMontColsJob):
    """An open typed batch in flight (dsv_verify_keyed_open_mont_cols_submit): MontColsJob's interface; reports no
    miss count.  Keeps the key set and the column arrays alive until the wait."""
    _symbol, _what = "dsv_verify_keyed_open_mont_cols_submit", "submit_open_mont_cols"
    _widths = staticmethod(lambda scheme: _layout(scheme, "_mont")[1])


def keyed_rlc_workspace_bytes(n, k, window_bits=0):
    """dsv_keyed_rlc_workspace_bytes: device bytes of KeySet.verify_rlc_dev's workspace for n items over k keys"""
    b = int(_lib.load().dsv_keyed_rlc_workspace_bytes(n, k, window_bits))
    if b == 0:
        raise ValueError("window_bits must be 0 or one of 4, 6, 8, 12, 14, 16")
    return b


def keyed_rlc_plan_info(scheme, n, k, window_bits=0, groups=1):
    """dsv_keyed_rlc_plan_info as a dict (no GPU needed): rlc_plan_info's fields for the keyed plan"""
    return _plan(_lib.load().dsv_keyed_rlc_plan_info, scheme, n, k, window_bits, groups)


def keyed_rlc_history(device=0, set_to=-1):
    """dsv_debug_keyed_rlc_history: the keyed calls' own history counter; returns the value before the call"""
    return _history(_lib.load().dsv_debug_keyed_rlc_history, device, set_to)


class KeySet:
    """Registered keys (dsv_keyset_*): per-key fixed-base tables on the device that is current when the set
    is built; verify by key index.  scheme: "single" (PK), "double" (PK, PK') or "vargen" (PK, Gen).

        ks = KeySet("single", PK)                  # PK: uint8 [k, 64] affine points
        ks = KeySet("double", PK, PKp)
        ks = KeySet.from_wire("vargen", pk64)      # the reference's key records, [k, 32] or [k, 64]
        ok = ks.verify(u, R, idx, m)               # double: ks.verify(u, R, Rp, idx, m); idx: uint32 [n]
        ks.verify_dev(u, R, idx, m, ok, workspace) # CUDA tensors; idx int32 [n], read as uint32
        ok = ks.verify_wire(sig, idx, m)           # sig: the reference's signature records, [n, 64] or [n, 96]
        ks.verify_wire_dev(sig, idx, m, ok, workspace)
        ks = KeySet.from_mont_cols("double", [pk96, pkp96])   # views into `PublicKey*` objects (limbs of u || v || z)
        ok = ks.verify_mont_cols([u, R96, idx, m])            # views into `Signature*` objects, where they lie
        job = ks.submit_mont_cols([u, R96, idx, m]); ok = job.wait()
        ks.verify_mont_dev(u, R96, idx, m, ok, workspace)     # CUDA tensors of limbs
        idx, misses = ks.lookup(PK)                # by key VALUE: uint32 [n], KEY_NONE where PK is not in the set
        ok, misses = ks.verify_lookup(u, R, PK, m) # closed-set verify; double: (u, R, Rp, PK, PKp, m); vargen:
        ks.verify_lookup_dev(u, R, PK, m, ok, workspace)      # (u, R, PK, Gen, m)
        ok, misses = ks.verify_open(u, R, PK, m)   # open-set verify (single, double): the unkeyed verdicts, a
        ks.verify_open_dev(u, R, PK, m, ok, workspace)        # registered key only makes them arrive sooner
        idx, misses = ks.lookup_wire(pk)           # by key RECORD ([n, 32] or [n, 64], as from_wire takes them)
        ok, misses = ks.verify_open_wire(sig, pk, m)          # open-set verify of serialized triples, every scheme:
        ks.verify_open_wire_dev(sig, pk, m, ok, workspace)    # the unkeyed wire verdicts; a hit needs no square root
        ks = KeySet.reserved("single", 4096, PK)   # room for 4096 keys (PK may be omitted: an empty set)
        first = ks.append(PK_new)                  # in place: indices first .. first + m - 1; append_wire(records),
        ks.k, ks.capacity                          # append_mont_cols([pk96]) for the other key forms
        ks.replace([3, 17], PK_two)                # eviction: new keys in the places of registered ones, in place;
        ks.replace_wire([5], record)               # k and every other key's index stay
        c = ks.census(PK)                          # the policy's input: c["hits"][j] items per registered key, and
        ks.census_dev(PK, idx, hits, rep, count, totals, workspace)   # the distinct missed keys as (rep, count)
    """

    def __init__(self, scheme, PK, PK2=None, _wire=None, _mont_cols=None, capacity=None):
        code = _code(scheme)
        self.scheme = scheme
        self._h = ctypes.c_void_p()
        L, out = _lib.load(), ctypes.byref(self._h)
        if capacity is not None and (_mont_cols is not None or _wire is not None):
            raise ValueError("capacity goes with affine keys: reserve, then append_wire / append_mont_cols")
        if capacity is not None and PK is None and PK2 is None:
            _lib.check(L.dsv_keyset_create_reserved(code, None, None, 0, capacity, out))
        elif _mont_cols is not None:
            k, arr, held = _keyed_columns(_mont_cols, [96] * _KEY_POINTS[scheme], "from_mont_cols")
            _lib.check(L.dsv_keyset_create_mont_cols(code, arr, k, out))
            del held
        elif _wire is not None:
            rec = _arr(_wire, self._rec_bytes())
            _lib.check(L.dsv_keyset_create_wire(code, _p(rec), rec.shape[0], out))
        else:
            k, keys = self._affine_keys(PK, PK2)
            if capacity is None:
                _lib.check(L.dsv_keyset_create(code, *_slots(_p(a) for a in keys), k, out))
            else:
                _lib.check(L.dsv_keyset_create_reserved(code, *_slots(_p(a) for a in keys), k, capacity, out))
        self._refresh()

    def _refresh(self):
        """k, capacity, nbytes, device from the library"""
        L = _lib.load()
        s, k, b, d, c = ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int(), ctypes.c_size_t()
        _lib.check(L.dsv_keyset_info(self._h, ctypes.byref(s), ctypes.byref(k), ctypes.byref(b), ctypes.byref(d)))
        _lib.check(L.dsv_keyset_capacity(self._h, ctypes.byref(c)))
        self.k, self.nbytes, self.device, self.capacity = k.value, b.value, d.value, c.value

    @classmethod
    def reserved(cls, scheme, capacity, PK=None, PK2=None):
        """dsv_keyset_create_reserved: the affine constructor with room for `capacity` keys; PK (and PK2) may be
        omitted for a set that starts empty.  append / append_wire / append_mont_cols register keys in place."""
        return cls(scheme, PK, PK2, capacity=int(capacity))

    def _affine_keys(self, PK, PK2):
        """keys as affine points (uint8 [m, 64]; PK2 for the two-point schemes) -> (m, their arrays)"""
        if (PK2 is None) != (self.scheme == "single"):
            raise ValueError("scheme %s takes %s"
                             % (self.scheme, "PK only" if self.scheme == "single" else "PK and PK2"))
        keys = [_arr(PK, 64)] + ([_arr(PK2, 64)] if PK2 is not None else [])
        return _same_n(*keys), keys

    def _appended(self, rc, first):
        _lib.check(rc)
        self._refresh()
        return int(first.value)

    def append(self, PK, PK2=None):
        """dsv_keyset_append: m more keys as affine points (uint8 [m, 64]; PK2 for the two-point schemes) into the
        live set, in place; blocks.  Returns the index of the first of them (the k before the call); calls enqueued
        afterwards see the new keys, calls in flight and captured graphs keep the k they were enqueued with."""
        m, keys = self._affine_keys(PK, PK2)
        first = ctypes.c_uint32()
        return self._appended(_lib.load().dsv_keyset_append(
            self._handle(), *_slots(_p(a) for a in keys), m, ctypes.byref(first)), first)

    def append_wire(self, pk_bytes):
        """dsv_keyset_append_wire: append() for the reference's key records ([m, 32] or [m, 64])"""
        rec = _arr(pk_bytes, self._rec_bytes())
        first = ctypes.c_uint32()
        return self._appended(_lib.load().dsv_keyset_append_wire(
            self._handle(), _p(rec), rec.shape[0], ctypes.byref(first)), first)

    def append_mont_cols(self, cols):
        """dsv_keyset_append_mont_cols: append() for key OBJECTS where they lie (cols as for from_mont_cols)"""
        m, arr, held = _keyed_columns(list(cols), [96] * _KEY_POINTS[self.scheme], "append_mont_cols")
        first = ctypes.c_uint32()
        rc = _lib.load().dsv_keyset_append_mont_cols(self._handle(), arr, m, ctypes.byref(first))
        del held
        return self._appended(rc, first)

    @staticmethod
    def _indices(indices, m):
        idx = np.ascontiguousarray(np.asarray(indices, dtype=np.uint32).reshape(-1))
        if idx.shape[0] != m:
            raise ValueError("%d indices for %d keys" % (idx.shape[0], m))
        return idx

    def replace(self, indices, PK, PK2=None):
        """dsv_keyset_replace: key j (affine points, uint8 [m, 64]; PK2 for the two-point schemes) takes the place
        of key indices[j] — pairwise distinct indices below k — in place; blocks.  k, the capacity and every other
        key's index stay; calls enqueued afterwards see the new keys.  No graph that holds the set may be replayed,
        and no stream of the device may be capturing, while it runs."""
        m, keys = self._affine_keys(PK, PK2)
        idx = self._indices(indices, m)
        _lib.check(_lib.load().dsv_keyset_replace(self._handle(), _p(idx), *_slots(_p(a) for a in keys), m))

    def replace_wire(self, indices, records):
        """dsv_keyset_replace_wire: replace() for the reference's key records ([m, 32] or [m, 64])"""
        rec = _arr(records, self._rec_bytes())
        idx = self._indices(indices, rec.shape[0])
        _lib.check(_lib.load().dsv_keyset_replace_wire(self._handle(), _p(idx), _p(rec), rec.shape[0]))

    @classmethod
    def from_wire(cls, scheme, pk_bytes):
        """from the reference's key records: PublicKey (32 B) / PublicKeyDouble / PublicKeyVarGen (64 B)"""
        return cls(scheme, None, _wire=pk_bytes)

    @classmethod
    def from_mont_cols(cls, scheme, cols):
        """from the reference's key OBJECTS where they lie (dsv_keyset_create_mont_cols): cols = [PK] (single),
        [PK, PK'] (double) or [PK, Gen] (vargen), each a uint8 [k, 96] view of the Montgomery limbs of u || v || z
        of a JubJubExtended (rows strided by the object size, bytes of a row contiguous)"""
        return cls(scheme, None, _mont_cols=list(cols))

    def _handle(self):
        if self._h.value is None:
            raise ValueError("key set is closed")
        return self._h

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value is not None:
            h, self._h = self._h, ctypes.c_void_p()
            _lib.check(_lib.load().dsv_keyset_destroy(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def key_ok(self):
        """one byte per registered key (dsv_keyset_key_ok_n): the buffer is sized by the capacity, which never
        changes, and cut to the k the library copied for — another thread's append may land at any time"""
        out = np.zeros(self.capacity, dtype=np.uint8)
        k = ctypes.c_size_t()
        _lib.check(_lib.load().dsv_keyset_key_ok_n(self._handle(), _p(out), out.shape[0], ctypes.byref(k)))
        return out[:min(k.value, out.shape[0])]

    def debug_entry(self, key, point, window, digit):
        """affine u || v of digit * 2^(8 * window) * point (0: PK, 1: PK' / Gen) from the key's table"""
        out = np.zeros(64, dtype=np.uint8)
        _lib.check(_lib.load().dsv_debug_keyset_entry(self._handle(), key, point, window, digit, _p(out)))
        return out

    # ---- the two bodies every verify method ends in ------------------------------------------------------------
    def _host_call(self, symbol, ins, n, misses=False):
        """symbol(ks, *ins, n, ok[, &misses]), a blocking host form -> verdicts [n] (misses: (verdicts, misses))"""
        ok = np.zeros(n, dtype=np.uint8)
        count = ctypes.c_size_t()
        tail = [ctypes.byref(count)] if misses else []
        _lib.check(getattr(_lib.load(), symbol)(self._handle(), *ins, n, _p(ok), *tail))
        return (ok, count.value) if misses else ok

    @staticmethod
    def _dev_tail(n, dev, ok, workspace, ws_need, stream):
        """what follows the inputs in every keyed _dev call, checked: n, ok, workspace, workspace_bytes, stream"""
        return [n, _bytes_out(ok, n, dev, "ok"), _bytes_out(workspace, ws_need, dev, "workspace"), workspace.numel(),
                _stream_ptr(stream, dev)]

    # ---- by key index ------------------------------------------------------------------------------------------
    def _pts(self, args):
        """(u, R[, Rp], idx, m) split by scheme"""
        want = 5 if self.scheme == "double" else 4
        if len(args) != want:
            raise ValueError("%s key set: verify takes %s" % (
                self.scheme, "(u, R, Rp, idx, m)" if want == 5 else "(u, R, idx, m)"))
        return args[0], args[1:-2], args[-2], args[-1]

    @staticmethod
    def _host_idx(idx, n):
        """the index column of the host forms: uint32 [n]"""
        idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
        if idx.shape[0] != n:
            raise ValueError("idx has %d entries, the batch %d items" % (idx.shape[0], n))
        return idx

    def verify(self, *args):
        """host arrays -> verdicts [n]; idx: key indices (uint32 [n]; an index >= k gives 0)"""
        u, pts, idx, m = self._pts(args)
        u, m = _arr(u, 32), _arr(m, 32)
        pts = [_arr(p, 64) for p in pts]
        n = _same_n(u, m, *pts)
        idx = self._host_idx(idx, n)
        return self._host_call("dsv_verify_%s_keyed" % self.scheme, [_p(u), *[_p(p) for p in pts], _p(idx), _p(m)], n)

    def _dev_args(self, args, what, width=64):
        """CUDA tensors (u, R[, Rp], idx, m, ok, workspace), points of `width` bytes, checked -> (n, dev, the input
        pointers in argument order, ok, workspace)"""
        if len(args) < 2:
            raise ValueError("%s takes the inputs, then ok and workspace" % what)
        ok, workspace = args[-2], args[-1]
        u, pts, idx, m = self._pts(args[:-2])
        names = ["u"] + ["R", "Rp"][:len(pts)] + ["m"]
        n, dev = _rows(*zip([u, *pts, m], [32] + [width] * len(pts) + [32], names))
        ip = _col32(idx, n, dev, "idx")
        return n, dev, [u.data_ptr(), *[p.data_ptr() for p in pts], ip, m.data_ptr()], ok, workspace

    def verify_dev(self, *args, stream=None):
        """CUDA tensors (u, R[, Rp], idx, m, ok, workspace): verdicts into ok, enqueued on `stream` (default:
        torch's current stream of the batch's device); does not synchronise.  idx: int32 [n], read as uint32;
        workspace: >= keyed_workspace_bytes(n) bytes."""
        n, dev, ins, ok, workspace = self._dev_args(args, "verify_dev")
        tail = self._dev_tail(n, dev, ok, workspace, keyed_workspace_bytes(n), stream)
        _lib.check(getattr(_lib.load(), "dsv_verify_%s_keyed_dev" % self.scheme)(self._handle(), *ins, *tail))

    def verify_rlc_dev(self, *args, stream=None, window_bits=0, accepted_out=None):
        """The keyed fast accept (dsv_verify_*_keyed_rlc_dev): the verdicts of verify_dev, through one aggregate
        test per group (or sub-group) when it is valid.  Same arguments; workspace: >=
        keyed_rlc_workspace_bytes(n, k, window_bits) bytes.  accepted_out None: the call waits for the stream and
        returns the accepted flag (bool); an int32 tensor on the batch's device or in pinned host memory: written
        by the device, the call does not block and returns None.  Never inside a graph capture (refused)."""
        n, dev, ins, ok, workspace = self._dev_args(args, "verify_rlc_dev")
        arg, box = _accepted_arg(accepted_out, dev)
        tail = self._dev_tail(n, dev, ok, workspace, keyed_rlc_workspace_bytes(n, self.k, window_bits), stream)
        _lib.check(getattr(_lib.load(), "dsv_verify_%s_keyed_rlc_dev" % self.scheme)(
            self._handle(), *ins, *tail, window_bits, arg))
        return bool(box.value) if box is not None else None

    def _sig_bytes(self):
        return _SCHEMES[self.scheme][1][0]

    def verify_wire(self, sig, idx, m):
        """Serialized signatures (dsv_verify_*_keyed_wire): host arrays sig [n, 64] (double: [n, 96]), idx
        uint32 [n], m [n, 32] -> verdicts [n], through the chunked host pipeline on the set's device."""
        sig, m = _arr(sig, self._sig_bytes()), _arr(m, 32)
        n = _same_n(sig, m)
        idx = self._host_idx(idx, n)
        return self._host_call("dsv_verify_%s_keyed_wire" % self.scheme, [_p(sig), _p(idx), _p(m)], n)

    def verify_wire_dev(self, sig, idx, m, ok, workspace, stream=None):
        """Serialized signatures in device memory (dsv_verify_*_keyed_wire_dev): CUDA tensors sig [n, 64]
        (double: [n, 96]), idx int32 [n] (read as uint32), m [n, 32]; verdicts into ok, enqueued on `stream`
        (default: torch's current stream of the batch's device); does not synchronise.  workspace: >=
        keyed_wire_workspace_bytes(scheme, n) bytes."""
        n, dev = _rows((sig, self._sig_bytes(), "sig"), (m, 32, "m"))
        ip = _col32(idx, n, dev, "idx")
        tail = self._dev_tail(n, dev, ok, workspace, keyed_wire_workspace_bytes(self.scheme, n), stream)
        _lib.check(getattr(_lib.load(), "dsv_verify_%s_keyed_wire_dev" % self.scheme)(
            self._handle(), sig.data_ptr(), ip, m.data_ptr(), *tail))

    def verify_mont_cols(self, cols):
        """`Signature*` objects where they lie (dsv_verify_keyed_mont_cols): cols = [u, R, idx, m] (double:
        [u, R, R', idx, m]), uint8 views [n, 32 | 96 | 4 | 32] of Montgomery limbs with strided rows (idx may be a
        uint32 [n] array or view) -> verdicts [n], through the chunked host pipeline on the set's device."""
        n, arr, held = _keyed_columns(cols, _keyed_mont_widths(self.scheme), "verify_mont_cols")
        ok = self._host_call("dsv_verify_keyed_mont_cols", [arr], n)
        del held
        return ok

    def submit_mont_cols(self, cols):
        """Asynchronous verify_mont_cols (dsv_verify_keyed_mont_cols_submit): returns a job at once (`wait()` ->
        verdicts, `done()`); the set cannot be destroyed or shut down under it."""
        return KeyedMontColsJob(self, cols)

    def verify_mont_dev(self, *args, stream=None):
        """Montgomery limbs in device memory (dsv_verify_keyed_mont_dev): CUDA tensors (u [n, 32], R [n, 96]
        [, Rp [n, 96]], idx int32 [n] read as uint32, m [n, 32], ok, workspace); verdicts into ok, enqueued on
        `stream` (default: torch's current stream of the batch's device); does not synchronise.  workspace: >=
        keyed_mont_workspace_bytes(scheme, n) bytes."""
        n, dev, ins, ok, workspace = self._dev_args(args, "verify_mont_dev", 96)
        tail = self._dev_tail(n, dev, ok, workspace, keyed_mont_workspace_bytes(self.scheme, n), stream)
        # one call for every scheme: (u, R, Rp or null, idx, m)
        _lib.check(_lib.load().dsv_verify_keyed_mont_dev(self._handle(), ins[0], *_slots(ins[1:-2]), *ins[-2:], *tail))

    # ---- by key value: the index over the set's own keys -----------------------------------------------------
    def _key_cols(self, keys, what):
        """(key_a[, key_b]) by scheme"""
        want = _KEY_POINTS[self.scheme]
        if len(keys) != want:
            raise ValueError("%s key set: %s takes %s" % (
                self.scheme, what, "key_a" if want == 1 else "key_a and key_b (PK' / Gen)"))
        return list(keys)

    def index_stats(self):
        """dsv_debug_keyset_index_stats: dict(capacity, occupied, displaced, longest_probe) of the set's index"""
        out = (ctypes.c_uint64 * 4)()
        _lib.check(_lib.load().dsv_debug_keyset_index_stats(self._handle(), out))
        return dict(zip(("capacity", "occupied", "displaced", "longest_probe"), (int(v) for v in out)))

    def lookup(self, *keys):
        """host arrays key_a [n, 64] (two-point sets: key_a, key_b) -> (idx uint32 [n], misses): the lowest index of
        a valid registered key with these bytes, KEY_NONE where there is none"""
        cols = [_arr(c, 64) for c in self._key_cols(keys, "lookup")]
        n = _same_n(*cols)
        idx = np.zeros(n, dtype=np.uint32)
        misses = ctypes.c_size_t()
        _lib.check(_lib.load().dsv_keyset_lookup(
            self._handle(), *_slots(_p(c) for c in cols), n, _p(idx), ctypes.byref(misses)))
        return idx, misses.value

    @staticmethod
    def _key_ptr(t, name):
        """a key column of the _dev forms: uint8 [n, 64], 16-byte aligned (the lookup reads it in 16-byte loads)"""
        if _t(t, 64, name).data_ptr() % 16:
            raise ValueError("%s: key columns must be 16-byte aligned" % name)
        return t.data_ptr()

    @staticmethod
    def _misses_ptr(misses, dev):
        if misses is None:
            return None
        return _idx(misses, 1, dev, "misses")

    def lookup_dev(self, *args, misses=None, stream=None):
        """CUDA tensors (key_a[, key_b], idx_out): idx_out int32 [n], written as uint32 (KEY_NONE = -1); misses
        (optional): a 32-bit CUDA tensor whose first element is set to the number of KEY_NONE items.  Enqueued on
        `stream` (default: torch's current stream of the batch's device); does not synchronise."""
        if len(args) < 1:
            raise ValueError("lookup_dev takes the key columns, then idx_out")
        cols, out = self._key_cols(args[:-1], "lookup_dev"), args[-1]
        names = ["key_a", "key_b"][:len(cols)]
        n, dev = _rows(*zip(cols, [64] * len(cols), names))
        op = _col32(out, n, dev, "idx_out")
        _lib.check(_lib.load().dsv_keyset_lookup_dev(
            self._handle(), *_slots(self._key_ptr(c, name) for c, name in zip(cols, names)), n, op,
            self._misses_ptr(misses, dev), _stream_ptr(stream, dev)))

    def _by_value(self, args, what, scheme=None):
        """(u, R[, Rp], key_a[, key_b], m) split by scheme (default: the set's) -> u, nonce points, key columns, m"""
        scheme = scheme or self.scheme
        ns, nk = (2 if scheme == "double" else 1), _KEY_POINTS[scheme]
        if len(args) != 2 + ns + nk:
            raise ValueError("%s key set: %s takes (%s)" % (self.scheme, what, ", ".join(_SCHEMES[scheme][0])))
        return args[0], list(args[1:1 + ns]), list(args[1 + ns:-1]), args[-1]

    @staticmethod
    def _value_ins(ptrs, ns, scheme):
        """the pointers (u, ns nonce points, the key columns, m) as a by-value call takes them.  scheme None: one
        of the calls that serve every scheme, with two places for the nonce points and two for the key columns
        (null where the set's scheme has one); else that scheme's own call, which takes exactly its columns"""
        if scheme is not None:
            return ptrs
        return [ptrs[0], *_slots(ptrs[1:1 + ns]), *_slots(ptrs[1 + ns:-1]), ptrs[-1]]

    def _verify_by_value(self, symbol, args, what, scheme=None):
        """a by-value verify over host arrays -> (verdicts [n], misses); scheme as for _value_ins"""
        u, pts, keys, m = self._by_value(args, what, scheme)
        u, m = _arr(u, 32), _arr(m, 32)
        pts, keys = [_arr(p, 64) for p in pts], [_arr(c, 64) for c in keys]
        n = _same_n(u, m, *pts, *keys)
        ins = self._value_ins([_p(a) for a in (u, *pts, *keys, m)], len(pts), scheme)
        return self._host_call(symbol, ins, n, misses=True)

    def _verify_by_value_dev(self, symbol, args, what, ws_bytes, misses, stream, width=64, scheme=None):
        """a by-value verify over CUDA tensors (..., ok, workspace), points of `width` bytes, workspace of
        ws_bytes(n) bytes; scheme as for _value_ins"""
        if len(args) < 2:
            raise ValueError("%s takes the inputs, then ok and workspace" % what)
        ok, workspace = args[-2], args[-1]
        u, pts, keys, m = self._by_value(args[:-2], what, scheme)
        names = ["u"] + ["R", "Rp"][:len(pts)] + ["key_a", "key_b"][:len(keys)] + ["m"]
        cols = list(zip([u, *pts, *keys, m], [32] + [width] * (len(pts) + len(keys)) + [32], names))
        n, dev = _rows(*cols)
        tail = self._dev_tail(n, dev, ok, workspace, ws_bytes(n), stream)
        if width == 96:  # the typed form reads every input in 16-byte loads, the affine forms the key columns
            ptrs = [self._rec_ptr(t, w, name) for t, w, name in cols]
        else:
            ptrs = [self._key_ptr(t, name) if name.startswith("key") else t.data_ptr() for t, w, name in cols]
        _lib.check(getattr(_lib.load(), symbol)(
            self._handle(), *self._value_ins(ptrs, len(pts), scheme), *tail, self._misses_ptr(misses, dev)))

    def verify_lookup(self, *args):
        """Closed-set verify by key value (dsv_verify_keyed_lookup): host arrays (u, R, PK, m) — double (u, R, Rp,
        PK, PKp, m), vargen (u, R, PK, Gen, m), the unkeyed entry points' arguments — -> (verdicts [n], misses).
        An item whose key is not a valid registered key of the set is rejected."""
        return self._verify_by_value("dsv_verify_keyed_lookup", args, "verify_lookup")

    def verify_lookup_dev(self, *args, misses=None, stream=None):
        """CUDA tensors (u, R[, Rp], key_a[, key_b], m, ok, workspace): verify_lookup's verdicts into ok, enqueued
        on `stream` (default: torch's current stream of the batch's device); does not synchronise.  workspace: >=
        keyed_lookup_workspace_bytes(n) bytes; misses as for lookup_dev."""
        self._verify_by_value_dev("dsv_verify_keyed_lookup_dev", args, "verify_lookup_dev",
                                  keyed_lookup_workspace_bytes, misses, stream)

    def verify_open(self, *args):
        """Open-set verify by key value (dsv_verify_keyed_open; single and double sets): host arrays (u, R, PK, m) —
        double (u, R, Rp, PK, PKp, m), the unkeyed entry points' arguments — -> (verdicts [n], misses).  The
        verdicts are the unkeyed entry point's for every input: the set is a key cache.  An item whose key is not
        a valid registered key is decided by the unkeyed equation in the same call; misses counts those."""
        return self._verify_by_value("dsv_verify_keyed_open", args, "verify_open")

    def verify_open_dev(self, *args, misses=None, stream=None):
        """CUDA tensors (u, R[, Rp], key_a[, key_b], m, ok, workspace): verify_open's verdicts into ok, enqueued
        on `stream` (default: torch's current stream of the batch's device) as one chain of launches; does not
        synchronise and may be captured.  workspace: >= keyed_open_workspace_bytes(n) bytes; misses as for
        lookup_dev."""
        self._verify_by_value_dev("dsv_verify_keyed_open_dev", args, "verify_open_dev",
                                  keyed_open_workspace_bytes, misses, stream)

    def verify_vargen_open(self, *args):
        """verify_vargen_open(u, R, PK, Gen, m) -> (verdicts [n], misses): the var-generator scheme's open-set
        verify by key value (dsv_verify_vargen_keyed_open; var-generator sets — verify_open refuses them), host
        arrays.  The verdicts are verify_vargen's for every input; an item whose (PK, Gen) bytes are not those of a
        valid registered key is decided by the unkeyed equation in the same call, and misses counts those."""
        return self._verify_by_value("dsv_verify_vargen_keyed_open", args, "verify_vargen_open", "vargen")

    def verify_vargen_open_dev(self, *args, misses=None, stream=None):
        """verify_vargen_open_dev(u, R, PK, Gen, m, ok, workspace, misses=None, stream=None): CUDA tensors;
        verify_vargen_open's verdicts into ok, enqueued on `stream` (default: torch's current stream of the batch's
        device) as one chain of launches; does not synchronise and may be captured.  workspace: >=
        keyed_open_workspace_bytes(n) bytes; misses as for lookup_dev."""
        self._verify_by_value_dev("dsv_verify_vargen_keyed_open_dev", args, "verify_vargen_open_dev",
                                  keyed_open_workspace_bytes, misses, stream, scheme="vargen")

    # ---- by key record: the index over the compressed records of the set's own keys ----------------------------
    def _rec_bytes(self):
        return _SCHEMES[self.scheme][1][1]

    @staticmethod
    def _rec_ptr(t, width, name):
        """a record column of the _dev forms: uint8 [n, width], 16-byte aligned (read in 16-byte loads)"""
        if _t(t, width, name).data_ptr() % 16:
            raise ValueError("%s: records must be 16-byte aligned" % name)
        return t.data_ptr()

    def lookup_wire(self, pk):
        """host array pk [n, 32] (two-point sets: [n, 64]) of key records -> (idx uint32 [n], misses): the lowest
        index of a valid registered key whose canonical record these bytes are, KEY_NONE where there is none"""
        rec = _arr(pk, self._rec_bytes())
        n = rec.shape[0]
        idx = np.zeros(n, dtype=np.uint32)
        misses = ctypes.c_size_t()
        _lib.check(_lib.load().dsv_keyset_lookup_wire(self._handle(), _p(rec), n, _p(idx), ctypes.byref(misses)))
        return idx, misses.value

    def lookup_wire_dev(self, pk, idx_out, misses=None, stream=None):
        """CUDA tensors pk [n, 32 | 64], idx_out int32 [n] (written as uint32, KEY_NONE = -1); misses as for
        lookup_dev.  Enqueued on `stream` (default: torch's current stream of the batch's device); does not
        synchronise."""
        n, dev = _rows((pk, self._rec_bytes(), "pk"))
        op = _col32(idx_out, n, dev, "idx_out")
        _lib.check(_lib.load().dsv_keyset_lookup_wire_dev(
            self._handle(), self._rec_ptr(pk, self._rec_bytes(), "pk"), n, op, self._misses_ptr(misses, dev),
            _stream_ptr(stream, dev)))

    def verify_open_wire(self, sig, pk, m):
        """Open-set verify of serialized triples (dsv_verify_*_keyed_open_wire; every scheme): host arrays sig
        [n, 64] (double: [n, 96]), pk [n, 32] (two-point sets: [n, 64]), m [n, 32] -> (verdicts [n], misses).  The
        verdicts are verify_*_wire's for every input; an item whose key record is not the canonical record of a
        valid registered key is decided by the unkeyed equation in the same call, and misses counts those."""
        sig, rec, m = _arr(sig, self._sig_bytes()), _arr(pk, self._rec_bytes()), _arr(m, 32)
        n = _same_n(sig, rec, m)
        return self._host_call("dsv_verify_%s_keyed_open_wire" % self.scheme, [_p(sig), _p(rec), _p(m)], n,
                               misses=True)

    def verify_open_wire_dev(self, sig, pk, m, ok, workspace, misses=None, stream=None):
        """CUDA tensors sig [n, 64 | 96], pk [n, 32 | 64], m [n, 32]: verify_open_wire's verdicts into ok, enqueued
        on `stream` (default: torch's current stream of the batch's device) as one chain of launches; does not
        synchronise and may be captured.  workspace: >= keyed_open_wire_workspace_bytes(scheme, n) bytes; misses
        as for lookup_dev."""
        sb, rb = self._sig_bytes(), self._rec_bytes()
        n, dev = _rows((sig, sb, "sig"), (pk, rb, "pk"), (m, 32, "m"))
        tail = self._dev_tail(n, dev, ok, workspace, keyed_open_wire_workspace_bytes(self.scheme, n), stream)
        _lib.check(getattr(_lib.load(), "dsv_verify_%s_keyed_open_wire_dev" % self.scheme)(
            self._handle(), self._rec_ptr(sig, sb, "sig"), self._rec_ptr(pk, rb, "pk"), m.data_ptr(), *tail,
            self._misses_ptr(misses, dev)))

    # ---- the key cache for typed objects: verify_batch's arguments, Montgomery limbs ---------------------------
    def verify_open_mont_cols(self, cols):
        """Open-set verify of typed objects where they lie (dsv_verify_keyed_open_mont_cols): cols as for
        verify_mont_cols of the module — single [u, R, PK, m], double [u, R, R', PK, PK', m], vargen [u, R, PK, Gen,
        m]; uint8 views [n, 32 | 96 | 32] of Montgomery limbs with strided rows — -> (verdicts [n], misses).  The
        verdicts are verify_mont_cols' for every input; an item whose normalised key is not a valid registered key
        is decided by the unkeyed equation in the same call, and misses counts those."""
        n, arr, held = _keyed_columns(cols, _layout(self.scheme, "_mont")[1], "verify_open_mont_cols")
        res = self._host_call("dsv_verify_keyed_open_mont_cols", [arr], n, misses=True)
        del held
        return res

    def submit_open_mont_cols(self, cols):
        """Asynchronous verify_open_mont_cols (dsv_verify_keyed_open_mont_cols_submit): returns a job at once
        (`wait()` -> verdicts, `done()`; no miss count); the set cannot be destroyed or shut down under it."""
        return KeyedOpenMontColsJob(self, cols)

    def verify_open_mont_dev(self, *args, misses=None, stream=None):
        """Montgomery limbs in device memory (dsv_verify_keyed_open_mont_dev): CUDA tensors (u [n, 32], R [n, 96]
        [, Rp], PK [n, 96][, PKp | Gen], m [n, 32], ok, workspace), every input 16-byte aligned; verify_*_mont_dev's
        verdicts into ok, enqueued on `stream` (default: torch's current stream of the batch's device) as one chain
        of launches; does not synchronise and may be captured.  workspace: >=
        keyed_open_mont_workspace_bytes(scheme, n) bytes; misses as for lookup_dev."""
        self._verify_by_value_dev("dsv_verify_keyed_open_mont_dev", args, "verify_open_mont_dev",
                                  lambda n: keyed_open_mont_workspace_bytes(self.scheme, n), misses, stream, width=96)

    # ---- the census: per-key hit counts and the distinct missed keys (what a key cache's policy reads) ----------
    def _census_host(self, symbol, ins, n):
        """a host census -> dict(idx, hits, rep, count, misses, unusable): idx uint32 [n] as lookup writes it, hits
        uint32 [capacity] (items per registered key, counted from zero), rep / count uint32 [distinct missed keys]
        (the lowest item index of the key and its items; by count descending, then rep ascending), misses = missed
        items, unusable = those of them without key bytes (typed form)"""
        idx, hits = np.zeros(n, dtype=np.uint32), np.zeros(self.capacity, dtype=np.uint32)
        rep, count = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        totals = (ctypes.c_size_t * 4)()
        _lib.check(getattr(_lib.load(), symbol)(self._handle(), *ins, n, _p(idx), _p(hits), _p(rep), _p(count), totals))
        d = int(totals[0])
        return dict(idx=idx, hits=hits, rep=rep[:d].copy(), count=count[:d].copy(), misses=int(totals[1]),
                    unusable=int(totals[2]))

    def census(self, *keys):
        """dsv_keyset_census: host arrays key_a [n, 64] (two-point sets: key_a, key_b) -> the census of the batch's
        keys against the set (see _census_host); blocks"""
        cols = [_arr(c, 64) for c in self._key_cols(keys, "census")]
        return self._census_host("dsv_keyset_census", _slots(_p(c) for c in cols), _same_n(*cols))

    def census_wire(self, pk):
        """dsv_keyset_census_wire: census() over key records ([n, 32], two-point sets [n, 64])"""
        rec = _arr(pk, self._rec_bytes())
        return self._census_host("dsv_keyset_census_wire", [_p(rec)], rec.shape[0])

    def census_mont_cols(self, cols):
        """dsv_keyset_census_mont_cols: census() over key OBJECTS where they lie (cols as for from_mont_cols: views
        [n, 96] of Montgomery limbs u || v || z with strided rows); keys are compared by their normalised bytes, an
        item with unusable limbs counts in misses and unusable and has no report entry"""
        n, arr, held = _keyed_columns(list(cols), [96] * _KEY_POINTS[self.scheme], "census_mont_cols")
        res = self._census_host("dsv_keyset_census_mont_cols", [arr], n)
        del held
        return res

    def _census_dev(self, symbol, key_ptrs, n, dev, outs, ws_need, stream):
        """the tail of a _dev census, checked: (idx_out, hits, rep, count, totals, workspace) — idx_out int32 [n] or
        None, hits a 32-bit tensor of >= capacity elements or None (ADDED to), rep / count 32-bit of >= n elements,
        totals 32-bit of >= 4, workspace uint8 of >= ws_need bytes"""
        if len(outs) != 6:
            raise ValueError("a census takes the key columns, then idx_out, hits, rep, count, totals, workspace")
        idx_out, hits, rep, count, totals, workspace = outs
        _lib.check(getattr(_lib.load(), symbol)(
            self._handle(), *key_ptrs, n, None if idx_out is None else _col32(idx_out, n, dev, "idx_out"),
            None if hits is None else _idx(hits, self.capacity, dev, "hits"), _idx(rep, n, dev, "rep"),
            _idx(count, n, dev, "count"), _idx(totals, 4, dev, "totals"),
            _bytes_out(workspace, ws_need, dev, "workspace"), workspace.numel(), _stream_ptr(stream, dev)))

    def census_dev(self, *args, stream=None):
        """dsv_keyset_census_dev: CUDA tensors (key_a[, key_b], idx_out, hits, rep, count, totals, workspace) — see
        _census_dev; workspace >= keyset_census_workspace_bytes(n) bytes.  Entries [0, totals[0]) of rep / count are
        the report, in no particular order; totals = (distinct missed keys, missed items, unusable items, 0).
        Enqueued on `stream` (default: torch's current stream of the batch's device) as one chain of launches; does
        not synchronise and may be captured."""
        cols = self._key_cols(args[:-6], "census_dev")
        names = ["key_a", "key_b"][:len(cols)]
        n, dev = _rows(*zip(cols, [64] * len(cols), names))
        self._census_dev("dsv_keyset_census_dev", _slots(self._key_ptr(c, nm) for c, nm in zip(cols, names)), n, dev,
                         args[-6:], keyset_census_workspace_bytes(n), stream)

    def census_wire_dev(self, pk, *outs, stream=None):
        """dsv_keyset_census_wire_dev: census_dev over key records pk [n, 32 | 64]"""
        n, dev = _rows((pk, self._rec_bytes(), "pk"))
        self._census_dev("dsv_keyset_census_wire_dev", [self._rec_ptr(pk, self._rec_bytes(), "pk")], n, dev, outs,
                         keyset_census_workspace_bytes(n), stream)

    def census_mont_dev(self, *args, stream=None):
        """dsv_keyset_census_mont_dev: census_dev over key objects' limbs (PK [n, 96][, PKp | Gen]), 16-byte aligned;
        workspace >= keyset_census_mont_workspace_bytes(scheme, n) bytes; totals[2] counts the items with unusable
        limbs"""
        cols = self._key_cols(args[:-6], "census_mont_dev")
        names = ["key_a", "key_b"][:len(cols)]
        n, dev = _rows(*zip(cols, [96] * len(cols), names))
        self._census_dev("dsv_keyset_census_mont_dev", _slots(self._rec_ptr(c, 96, nm) for c, nm in zip(cols, names)),
                         n, dev, args[-6:], keyset_census_mont_workspace_bytes(self.scheme, n), stream)
