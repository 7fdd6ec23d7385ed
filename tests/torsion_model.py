"""A point of order 8 on JubJub (Python integers, CPU): the small-order component the torsion cases of the CPU
models, the GPU suites and tools/soak_rlc.py add to keys, generators and nonce points.  `rnd` is the one stream
those callers share; tests/test_halfgcd.py passes its own."""
import random

import pymodel as M

rnd = random.Random(2024)


def _sqrt(n, p=M.Q):
    q, s = p - 1, 0
    while q % 2 == 0:
        q //= 2
        s += 1
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    m, c, t, r = s, pow(z, q, p), pow(n, q, p), pow(n, (q + 1) // 2, p)
    while t != 1:
        i, tt = 0, t
        while tt != 1:
            tt = tt * tt % p
            i += 1
        b = pow(c, 1 << (m - i - 1), p)
        m, c, t, r = i, b * b % p, t * b * b % p, r * b % p
    return r


def order8_point(rnd=rnd):
    while True:
        v = rnd.randrange(M.Q)
        u2 = (v * v - 1) * pow(1 + M.D * v * v, -1, M.Q) % M.Q
        if pow(u2, (M.Q - 1) // 2, M.Q) != 1:
            continue
        p = (_sqrt(u2), v)
        assert M.on_curve(p)
        t = M.pmul(p, M.R_ORDER)
        if M.pmul(t, 4) != M.IDENTITY:
            return t
