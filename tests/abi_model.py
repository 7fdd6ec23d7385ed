"""What the CPU-side ABI tests share: the symbols include/dsv.h declares, and the size model of a key set's index
(points per key, 256-byte rounding, the slot-table capacity)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dsv.h")
POINTS = {"single": 1, "double": 2, "vargen": 2}


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dsv_[a-z0-9_]+)\s*\(", text)))


def _up(x, a=256):
    return (x + a - 1) // a * a


def cap_of(k):
    """the smallest power of two >= max(64, 2k)"""
    cap = 64
    while cap < 2 * k:
        cap *= 2
    return cap
