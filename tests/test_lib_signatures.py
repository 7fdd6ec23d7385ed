"""CPU test of the binding's signature table: every prototype of include/dsv.h, mapped to ctypes by one rule,
must be what _lib.load() set as argtypes / restype of that symbol.  The package itself never reads the header."""
import ctypes
import os
import re

from schnorr_amd import _lib
from abi_model import HEADER, declared_symbols

SCALARS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64}
PROTOTYPE = re.compile(r"\b((?:const\s+)?\w+(?:\s*\*)?)\s*(dsv_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")


def ctype_of(decl, where):
    """the ctypes type of one C result or parameter declaration (the parameter's name, if any, included)"""
    decl = " ".join(decl.split())
    if "*" in decl or "[" in decl:
        return ctypes.c_char_p if re.match(r"const char ?\*", decl) else ctypes.c_void_p
    words = decl.split()
    assert words and words[0] in SCALARS, "%s: type %r is outside the binding's mapping" % (where, decl)
    return SCALARS[words[0]]


def prototypes():
    """{name: (restype, [argtypes])} of every function include/dsv.h declares"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    found = {}
    for result, name, params in PROTOTYPE.findall(text):
        assert name not in found, "%s is declared twice" % name
        params = [] if params.strip() == "void" else params.split(",")
        found[name] = (ctype_of(result, name + " (result)"),
                       [ctype_of(p, "%s (parameter %d)" % (name, k)) for k, p in enumerate(params)])
    return found


def test_every_prototype_is_found():
    protos = prototypes()
    assert len(protos) >= 182
    assert sorted(protos) == declared_symbols() == sorted(_lib.SYMBOLS)


def test_signatures_match_the_header():
    L = _lib.load()
    wrong = []
    for name, (restype, argtypes) in sorted(prototypes().items()):
        fn = getattr(L, name)
        if fn.restype is not restype or list(fn.argtypes or ()) != argtypes or fn.argtypes is None:
            wrong.append(name)
    assert not wrong, "argtypes / restype differ from include/dsv.h: %s" % ", ".join(wrong)


def test_pointer_parameters_refuse_what_ctypes_would_truncate():
    """what the table is for: a numpy integer or a c_size_t given for a pointer raises, None and ints pass"""
    import numpy as np
    import pytest

    vp = _lib.load().dsv_job_done.argtypes[0]
    assert vp is ctypes.c_void_p
    for good in (None, 0, 1 << 40, ctypes.c_void_p(5), ctypes.byref(ctypes.c_int()), (ctypes.c_uint8 * 4)()):
        vp.from_param(good)
    for bad in (np.int64(5), ctypes.c_size_t(5)):
        with pytest.raises((TypeError, ctypes.ArgumentError)):
            vp.from_param(bad)
