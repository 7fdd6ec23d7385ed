"""The hand-off check of reference fixtures (tests/reference_fixtures.py), shared by its CPU form on the oracle
(tests/test_oracle.py) and its GPU form on the HIP engine (tests/test_gpu_parity.py)."""
import ctypes

import numpy as np

import harness as H
import oracle_lib as O
import pymodel as M

unhex = lambda s: np.frombuffer(bytes.fromhex(s), dtype=np.uint8)


class Backend:
    """the functions a fixture check drives: the oracle's (CPU) or the HIP engine's (GPU)"""
    def __init__(self, mod, decompress, stdrng=None):
        for k in ("verify_single", "verify_double", "verify_vargen", "verify_single_wire", "verify_double_wire",
                  "verify_vargen_wire", "challenge_single", "challenge_double"):
            setattr(self, k, getattr(mod, k))
        self.decompress = decompress
        self.stdrng = stdrng          # engine only: (seed, n) -> (sk, m, nonce) of the GPU's own ChaCha12


ORACLE_BACKEND = Backend(O, O.decompress)


def _check_reference_records(recs, be=ORACLE_BACKEND):
    """shared by the CPU (oracle) and GPU (engine) forms of the hand-off test; returns the number
    of records checked per kind"""
    import refrng
    from collections import Counter
    seen = Counter()
    row = lambda h, w: unhex(h).reshape(1, w)
    for r in recs:
        k = r["kind"]
        seen[k] += 1
        if k == "sponge_hash":
            assert M.le32(M.sponge_hash(list(range(1, r["n"] + 1)))).hex() == r["hex"], \
                "Poseidon sponge of %d inputs differs from the crate" % r["n"]
        elif k == "truncated_hash":
            assert M.le32(M.truncated_hash(list(range(1, r["n"] + 1)))).hex() == r["hex"], \
                "250-bit truncated hash of %d inputs differs" % r["n"]
        elif k == "sig":
            u, m = row(r["u"], 32), row(r["m"], 32)
            R, PK = row(r["R"], 64), row(r["PK"], 64)
            assert int(be.verify_single(u, R, PK, m)[0]) == int(r["verdict"]), ("verdict", r["i"])
            sig, pk = row(r["sig_bytes"], 64), row(r["pk_bytes"], 32)
            assert int(be.verify_single_wire(sig, pk, m)[0]) == int(r["verdict"]), ("wire verdict", r["i"])
            if "c" in r:
                assert bytes(be.challenge_single(R, m)[0]).hex() == r["c"], ("challenge", r["i"])
            # the crate's own PK = sk * G and serialisation
            sk = M.from_le(unhex(r["sk"]))
            assert M.point_bytes(M.pmul(M.GEN, sk)).hex() == r["PK"], ("PK = sk*G", r["i"])
            assert M.compress(H.to_int_point(PK[0])).hex() == r["pk_bytes"]
            assert r["sig_bytes"] == r["u"] + M.compress(H.to_int_point(R[0])).hex()
        elif k == "sigd":
            u, m = row(r["u"], 32), row(r["m"], 32)
            R, Rp, PK, PKp = (row(r[x], 64) for x in ("R", "Rp", "PK", "PKp"))
            assert int(be.verify_double(u, R, Rp, PK, PKp, m)[0]) == int(r["verdict"]), ("verdict", r["i"])
            assert int(be.verify_double_wire(row(r["sig_bytes"], 96), row(r["pk_bytes"], 64), m)[0]) == \
                int(r["verdict"]), ("wire verdict", r["i"])
            assert bytes(be.challenge_double(R, Rp, m)[0]).hex() == r["c"], ("double challenge", r["i"])
            sk = M.from_le(unhex(r["sk"]))
            assert M.point_bytes(M.pmul(M.GEN, sk)).hex() == r["PK"], ("PK = sk*G", r["i"])
            assert M.point_bytes(M.pmul(M.GEN_NUMS, sk)).hex() == r["PKp"], ("PK' = sk*G'", r["i"])
            comp = lambda x: M.compress(H.to_int_point(x[0])).hex()
            assert r["pk_bytes"] == comp(PK) + comp(PKp) and r["sig_bytes"] == r["u"] + comp(R) + comp(Rp)
        elif k == "sigv":
            u, m = row(r["u"], 32), row(r["m"], 32)
            R, PK, Gen = (row(r[x], 64) for x in ("R", "PK", "Gen"))
            assert int(be.verify_vargen(u, R, PK, Gen, m)[0]) == int(r["verdict"]), ("verdict", r["i"])
            assert int(be.verify_vargen_wire(row(r["sig_bytes"], 64), row(r["pk_bytes"], 64), m)[0]) == \
                int(r["verdict"]), ("wire verdict", r["i"])
            assert bytes(be.challenge_single(R, m)[0]).hex() == r["c"], ("challenge", r["i"])
            comp = lambda x: M.compress(H.to_int_point(x[0])).hex()
            # SecretKeyVarGen::to_bytes = sk || compressed generator; PublicKeyVarGen = pk || generator
            sk = M.from_le(unhex(r["sk_bytes"][:64]))
            assert r["sk_bytes"][64:] == comp(Gen) and r["pk_bytes"] == comp(PK) + comp(Gen)
            assert M.point_bytes(M.pmul(H.to_int_point(Gen[0]), sk)).hex() == r["PK"], ("PK = sk*Gen", r["i"])
            assert r["sig_bytes"] == r["u"] + comp(R)
        elif k == "stdrng":
            assert refrng.StdRng(r["seed"]).fill_bytes(r["n"]).hex() == r["hex"], "StdRng keystream differs"
            if be.stdrng and r["n"] >= 192:
                sk, m, nonce = be.stdrng(r["seed"], r["n"] // 192)
                raw = bytes.fromhex(r["hex"])
                for i in range(r["n"] // 192):
                    w = [int.from_bytes(raw[192 * i + 64 * j:192 * i + 64 * j + 64], "little") for j in range(3)]
                    assert (M.from_le(sk[i]), M.from_le(m[i]), M.from_le(nonce[i])) == \
                        (w[0] % M.R_ORDER, w[1] % M.Q, w[2] % M.R_ORDER)
        elif k == "wide":
            v = int.from_bytes(bytes.fromhex(r["wide"]), "little")
            mod = M.R_ORDER if r["field"] == "fr" else M.Q
            assert M.le32(v % mod).hex() == r["hex"], "from_bytes_wide / Field::random differs"
            # the oracle's own wide reduction (lo * R^2 + hi * R^3), through its keygen entry point
            if r["field"] == "fr":
                w = unhex(r["wide"]).reshape(1, 64)
                d = {x: np.zeros((1, s), np.uint8) for x, s in (("sk", 32), ("m", 32), ("u", 32), ("R", 64), ("PK", 64))}
                O.lib().oracle_keygen_sign_single(O._p(w), O._p(w), O._p(w), ctypes.c_size_t(1), O._p(d["sk"]),
                                                  O._p(d["m"]), O._p(d["u"]), O._p(d["R"]), O._p(d["PK"]), ctypes.c_int(1))
                assert bytes(d["sk"][0]).hex() == r["hex"]
        elif k == "from_bytes":
            out, ok = be.decompress(unhex(r["enc"]).reshape(1, 32))
            assert bool(ok[0]) == r["ok"], ("from_bytes accept/reject", r["i"])
            if r["ok"]:
                assert bytes(out[0]).hex() == r["u"] + r["v"], ("from_bytes value", r["i"])
        else:
            raise AssertionError("unknown record kind %r" % k)
    return seen
