"""The joint 2-bit window table of k_verify_fixed_half as read from the source (schnorr_amd/csrc/common.h:
joint_slot, recode_signed2): the slot contents, the digit-pair -> signed-slot map and the recoding, on Python
integers.  Shared by tests/test_joint_windows.py and tests/test_gpu_table_layout.py."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "schnorr_amd", "csrc", "common.h")).read()

# (coefficient of P, coefficient of R) held by each slot, as build_joint_table fills them
SLOT = {1: (1, 0), 2: (0, 1), 3: (2, 0), 4: (0, 2), 5: (1, 1), 6: (1, -1), 7: (2, 1), 8: (2, -1),
        9: (1, 2), 10: (-1, 2), 11: (2, 2)}
A = int("55" * 32, 16)   # bias: digit = 2-bit field - 1, in [-1, 2]
BIAS = 1


def _constants():
    slots = int(re.search(r"slots = (0x[0-9A-Fa-f]+)ULL", SRC).group(1), 16)
    neg = int(re.search(r"\(\((0x[0-9A-Fa-f]+)u >> idx\) & 1u\)", SRC).group(1), 16)
    return slots, neg


def joint_slot(ra, rb):
    slots, neg = _constants()
    idx = ra * 4 + rb
    s = (slots >> (4 * idx)) & 15
    return -s if (neg >> idx) & 1 else s


def recode_signed2(s):
    y = A + s
    assert 0 <= y < 1 << 256
    return y
