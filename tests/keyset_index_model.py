"""A Python model of the canonical layout of a key set's indices (include/dsv.h, "keys replaced in place"; DESIGN.md
§10.8): the slot array that inserting key 0, then 1, and so on gives — each valid key that equals no valid key of
lower index goes into the first empty slot from its home slot on, wrapping.  Home slots come from the library's own
introspection calls (no GPU needed), everything else is plain Python."""
import numpy as np

NONE = 0xFFFFFFFF
FORMS = ("affine", "record")


def cap_of(capacity):
    """slots of a set of `capacity` keys: the smallest power of two >= max(64, 2 * capacity)"""
    cap = 64
    while cap < 2 * capacity:
        cap *= 2
    return cap


def record_of(P):
    """the compressed record of affine points u || v ([n, 64]) by byte operations: v, bit 255 = the lowest bit of u"""
    P = np.asarray(P, dtype=np.uint8).reshape(-1, 64)
    rec = P[:, 32:].copy()
    rec[:, 31] = (rec[:, 31] & 0x7F) | ((P[:, 0] & 1) << 7)
    return rec


def records_of(P0, P1=None):
    """key records of affine keys: 32 B per key point"""
    return np.ascontiguousarray(record_of(P0) if P1 is None else np.hstack([record_of(P0), record_of(P1)]))


def home_slot(E, scheme, capacity, form, a, b=None):
    """the home slot of the key a [, b] (affine bytes) in the `form` index of a set of `capacity` keys"""
    if form == "affine":
        return E.keyset_home_slot(scheme, capacity, a, b)
    return E.keyset_wire_home_slot(scheme, capacity, records_of(a, b))


def canonical_slots(E, scheme, P0, P1, key_ok, capacity, form, homes=None):
    """uint32 [cap_of(capacity)]: sequential insertion of keys 0 .. len(P0) - 1 in index order, keys with key_ok == 0
    left out, of equal keys (equal affine bytes: for valid keys the same as equal records) only the lowest index.
    homes (optional): the keys' home slots, for callers that know them"""
    assert form in FORMS
    cap = cap_of(capacity)
    slots = np.full(cap, NONE, dtype=np.uint32)
    seen = set()
    for j in range(len(P0)):
        if not key_ok[j]:
            continue
        row = bytes(P0[j]) + (bytes(P1[j]) if P1 is not None else b"")
        if row in seen:
            continue
        seen.add(row)
        s = int(homes[j]) if homes is not None else home_slot(E, scheme, capacity, form, P0[j],
                                                                 P1[j] if P1 is not None else None)
        assert 0 <= s < cap
        while slots[s] != NONE:
            s = (s + 1) % cap
        slots[s] = j
    return slots


def check_ordered(slots, homes):
    """the invariant that makes the layout unique and the stale-k rule hold for every k: every slot between a key's
    home and its place holds a lower index.  homes: {index: home slot} of the occupants."""
    cap = len(slots)
    for p in range(cap):
        x = int(slots[p])
        if x == NONE:
            continue
        s = homes[x]
        while s != p:
            assert slots[s] != NONE and int(slots[s]) < x, (p, x, s, int(slots[s]))
            s = (s + 1) % cap
