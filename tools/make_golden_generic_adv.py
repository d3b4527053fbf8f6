"""tests/golden/bign_generic_adv.json: ADVERSARIAL moduli and parameter sets for the general-curve kernels
(bee2_amd/csrc/bign_generic_kernels.hip), the cases that reach the exceptional branches of their verification ladder, and
signing-side records.  Build container only: every verification code is the reference's (oracle/_ref/libbee2ref.so) and
is cross-checked with the Python restatement (tests/orc_generic.py) before the file is written; the tests read the file.

Moduli, per l in {128, 192, 256}:
  * primes p = 3 (mod 4): the smallest and the largest 2l-bit one, one with low limb 0xFFFFFFFF (n0 = 1), one with low limb
    3, one with an interior all-zero 32-bit limb, one with an interior all-ones limb, one random;
  * odd moduli q (not necessarily prime: bignParamsCheck does not ask): 2^(2l) - 1, 2^(2l-1) + 1, one with low limb 1
    (n0 = 0xFFFFFFFF), one random.  The reference accepts each as the q of a parameter set or it is dropped from "sets".
Parameter sets ("sets"):
  * "adv": one per prime, random a and yG, b = yG^2, the q's above in turn.  q is NOT the group order; valid signatures
    exist all the same (tools/make_golden_generic.py): with d < 2^(l-2) and k >= 2^(2l-1), u = k - (s0 + 2^l) d is a
    non-negative integer below q and s1 = (u - H) mod q verifies whatever the order of G is -- with a full-size hash;
  * "tors": a curve with the rational 2-torsion point (x0, 0): b = -(x0^3 + a x0), a non-zero square, yG = b^((p+1)/4);
  * "iso": a fresh image of the standard curve, (a, b, yG) -> (t^4 a, t^6 b, t^3 yG): q IS the group order (odd, prime).
"crafted": signatures that drive the simultaneous double-and-add of the verification kernel into gj_add's T == E and
T == -E branches, gj_dbl's Y == 0 branch and R == O (tests/test_gpu_bign_generic.py names each case and models the ladder).
"pubkey_calc" / "sign_k": on the iso sets, produced by the reference (bignPubkeyCalc; bignSign with a generator that
replays k); on the other sets by tests/orc_generic.py ("by": "python"), the reference's scalar recoding needing the true
group order (tools/make_golden_generic_sign.py).
"""
import ctypes
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import refgen  # noqa: E402
import orc_generic as OG  # noqa: E402
import make_golden_sign as MS  # noqa: E402
from make_golden_generic import STD, hexp, is_prime, mk, ref_belt_hash, ref_verify, std  # noqa: E402
from bee2_amd.engine import LEVEL_OID  # noqa: E402

L = refgen.ref()
_sz = ctypes.c_size_t


def prime_from(rnd, start, step):
    p = start
    while p % 4 != 3 or not is_prime(p, rnd):
        p += step
    return p


def prime_shaped(rnd, l, shape):
    """random 2l-bit prime = 3 (mod 4) after `shape` has fixed some limbs"""
    while True:
        p = shape(rnd.getrandbits(2 * l) | (1 << (2 * l - 1)))
        if p % 4 == 3 and p >> (2 * l - 1) == 1 and is_prime(p, rnd):
            return p


def moduli(rnd, l):
    n = l // 16
    j = n // 2
    limb = 0xFFFFFFFF
    primes = [
        ("smallest", prime_from(rnd, (1 << (2 * l - 1)) + 3, 4)),
        ("largest", prime_from(rnd, (1 << (2 * l)) - 1, -4)),
        ("low limb ffffffff", prime_shaped(rnd, l, lambda x: x | limb)),
        ("low limb 3", prime_shaped(rnd, l, lambda x: (x >> 32 << 32) | 3)),
        ("interior zero limb", prime_shaped(rnd, l, lambda x: (x & ~(limb << (32 * j))) | 3)),
        ("interior ones limb", prime_shaped(rnd, l, lambda x: x | (limb << (32 * j)) | 3)),
        ("random", prime_shaped(rnd, l, lambda x: x | 3)),
    ]
    top = 1 << (2 * l - 1)
    odd = [
        ("2^(2l) - 1", (1 << (2 * l)) - 1),
        ("2^(2l-1) + 1", top + 1),
        ("low limb 1", ((rnd.getrandbits(2 * l) | top) >> 32 << 32) | 1),
        ("random odd", rnd.getrandbits(2 * l) | top | 1),
    ]
    return primes, odd


def sqrt34(x, p):
    y = pow(x, (p + 1) // 4, p)
    return y if y * y % p == x % p else None


def nowrap_sig(rnd, l, p, a, q, yG, oid, d, h, k):
    """(sig, R) with u = k - (s0 + 2^l) d taken over the integers; None unless 0 <= u < q"""
    no = l // 4
    R = OG.mul(k, (0, yG), a, p)
    s0 = ref_belt_hash(oid + R[0].to_bytes(no, "little") + h)[:no // 2]
    u = k - (OG.le(s0) + (1 << l)) * d
    if not 0 <= u < q:
        return None
    H = OG.le(h)
    if H >= q:
        H -= q
    return s0 + ((u - H) % q).to_bytes(no, "little")


def crafted(rnd, P, l, p, a, q, yG, x0, oid):
    """the five exceptional cases: (name, hash, sig, pubkey) -- see tests/test_gpu_bign_generic.py for why each reaches its branch"""
    no = l // 4
    G = (0, yG)
    enc = lambda Q: Q[0].to_bytes(no, "little") + Q[1].to_bytes(no, "little")
    out = []
    negG = (0, p - yG)
    G2 = OG._add(G, G, a, p)
    for name, Q, d, kf, cnt in (("T == E", G, 1, lambda t: 3 * (1 << l) + t, 2), ("T == -E", negG, -1, lambda t: t, 2),
                                ("T == E later", G2, 2, lambda t: 5 * (1 << l) + t, 4)):
        for _ in range(cnt):
            h = rnd.randbytes(no)
            k = kf(rnd.getrandbits(l - 10) | 1)
            sig = nowrap_sig(rnd, l, p, a, q, yG, oid, d, h, k)
            assert sig is not None
            if name.split(" later")[0].replace("T", "add T", 1) in {e for e, _ in OG.ladder_events(P, h, sig, enc(Q))}:
                out.append((name, h, sig, enc(Q)))
        assert [x for x in out if x[0] == name], name
    if x0 is not None:                                      # parity forgery under the key of order 2
        Q = (x0, 0)
        done = 0
        while done < 2:
            u = rnd.getrandbits(l - 1) | 1
            h = rnd.randbytes(no)
            for par in (0, 1):
                R = OG._add(OG.mul(u, G, a, p), Q if par else None, a, p)
                s0 = ref_belt_hash(oid + R[0].to_bytes(no, "little") + h)[:no // 2]
                if s0[0] & 1 == par:
                    H = OG.le(h)
                    if H >= q:
                        H -= q
                    out.append(("Y == 0 doubling", h, s0 + ((u - H) % q).to_bytes(no, "little"), enc(Q)))
                    done += 1
                    break
    for h in (bytes(no), q.to_bytes(no, "little")):         # H = 0 (mod q), s1 = s0 + 2^l: u = v and Q = -G
        s0 = rnd.randbytes(no // 2)
        out.append(("R == O", h, s0 + (OG.le(s0) + (1 << l)).to_bytes(no, "little"), enc(negG)))
    return out


def main():
    rnd = random.Random(0x616476)
    out = {"moduli": [], "sets": [], "verify": [], "crafted": [], "pubkey_calc": [], "sign_k": []}
    for l in (128, 192, 256):
        no = l // 4
        oid = bytes(LEVEL_OID[l])
        primes, odd = moduli(rnd, l)
        for kind, m in primes:
            out["moduli"].append({"l": l, "kind": kind, "prime": True, "m": m.to_bytes(no, "little").hex()})
        for kind, m in odd:
            out["moduli"].append({"l": l, "kind": kind, "prime": False, "m": m.to_bytes(no, "little").hex()})
        sets = []
        for i, (kind, p) in enumerate(primes):
            a, yG = rnd.randrange(1, p), rnd.randrange(1, p)
            sets.append(("adv", kind, p, a, yG * yG % p, odd[i % 4], yG, None))
        p = primes[6][1]
        while True:
            a, x0 = rnd.randrange(1, p), rnd.randrange(1, p)
            b = -(x0 ** 3 + a * x0) % p
            yG = sqrt34(b, p) if b else None
            if yG:
                break
        sets.append(("tors", "random", p, a, b, odd[3], yG, x0))
        base = std(STD[l])
        p, a, b, q, yG = (OG.le(bytes(getattr(base, f))[:no]) for f in ("p", "a", "b", "q", "yG"))
        t = rnd.randrange(2, p)
        sets.append(("iso", "standard", p, a * pow(t, 4, p) % p, b * pow(t, 6, p) % p, ("standard", q), yG * pow(t, 3, p) % p, None))

        for kind, pkind, p, a, b, (qkind, q), yG, x0 in sets:
            prm = mk(l, p, a, b, q, yG)
            P = OG.Params.from_hex(hexp(prm))
            G = (0, yG)
            # the reference has to take the set: a valid signature verifies, or the set is dropped
            d = rnd.getrandbits(l - 2) | 1
            Q = OG.mul(d, G, a, p)
            pub = Q[0].to_bytes(no, "little") + Q[1].to_bytes(no, "little")
            probe_h = rnd.randbytes(no)
            probe = nowrap_sig(rnd, l, p, a, q, yG, oid, d, probe_h, rnd.getrandbits(2 * l - 1) | (1 << (2 * l - 1))) if kind != "iso" else None
            if probe is not None and ref_verify(prm, oid, probe_h, probe, pub) != 0:
                print("dropped:", l, kind, pkind, qkind, ref_verify(prm, oid, probe_h, probe, pub))
                continue
            si = len(out["sets"])
            ent = {"kind": kind, "p_kind": pkind, "q_kind": qkind, **hexp(prm)}
            if x0 is not None:
                ent["x0"] = x0.to_bytes(no, "little").hex()
            out["sets"].append(ent)

            def put(where, name, h, s, k):
                code = ref_verify(prm, oid, bytes(h), bytes(s), bytes(k)) & 0xFFFFFFFF
                assert code == OG.verify(P, oid, bytes(h), bytes(s), bytes(k), ref_belt_hash), (l, kind, name)
                out[where].append({"set": si, "name": name, "oid": oid.hex(), "hash": bytes(h).hex(), "sig": bytes(s).hex(),
                                   "pubkey": bytes(k).hex(), "code": code})
                return code

            # ---- valid signatures and their single-bit corruptions
            for rep in range(2):
                h = rnd.randbytes(no)
                if kind == "iso":
                    dd = rnd.randrange(1, q)
                    code, pub = OG.pubkey_calc(P, dd.to_bytes(no, "little"))
                    code, sig = OG.sign_k(P, oid, h, dd.to_bytes(no, "little"), rnd.randrange(1, q).to_bytes(no, "little"), ref_belt_hash)
                    assert code == 0
                else:
                    if rep == 1:
                        h = rnd.randrange(q, 1 << (2 * l)).to_bytes(no, "little") if q + 1 < 1 << (2 * l) else h
                    sig = nowrap_sig(rnd, l, p, a, q, yG, oid, d, h, rnd.getrandbits(2 * l - 1) | (1 << (2 * l - 1)))
                    if sig is None:
                        sig = nowrap_sig(rnd, l, p, a, q, yG, oid, d, h, 1 << (2 * l - 1))
                assert put("verify", "good", h, sig, pub) == 0
                if rep == 0:
                    x = bytearray(sig); x[rnd.randrange(no // 2)] ^= 1 << rnd.randrange(8); put("verify", "s0 bit", h, x, pub)
                    x = bytearray(sig); x[no // 2 + rnd.randrange(no)] ^= 1 << rnd.randrange(8); put("verify", "s1 bit", h, x, pub)
                    x = bytearray(h); x[rnd.randrange(no)] ^= 1 << rnd.randrange(8); put("verify", "hash bit", x, sig, pub)
            # ---- the exceptional branches of the ladder
            if kind in ("tors", "iso"):
                for name, h, s, k in crafted(rnd, P, l, p, a, q, yG, x0, oid):
                    put("crafted", name, h, s, k)
            # ---- signing side: by the reference where q is the group order
            if kind == "iso":
                ds = [rnd.randrange(1, q) for _ in range(3)] + [0, 1, 2, q - 1, q, (1 << (2 * l)) - 1]
                for dd in ds:
                    dbytes = dd.to_bytes(no, "little")
                    buf = ctypes.create_string_buffer(2 * no)
                    code = L.bignPubkeyCalc(buf, ctypes.byref(prm), dbytes) & 0xFFFFFFFF
                    assert (code, buf.raw if code == 0 else b"") == OG.pubkey_calc(P, dbytes)
                    out["pubkey_calc"].append({"set": si, "by": "reference", "priv": dbytes.hex(), "code": code, "pub": buf.raw.hex() if code == 0 else ""})
                hq = [rnd.randbytes(no), q.to_bytes(no, "little"), ((1 << (2 * l)) - 1).to_bytes(no, "little"), bytes(no)]
                for i, (dd, kk) in enumerate([(ds[0], rnd.randrange(1, q)), (ds[1], 1), (ds[2], q - 1), (1, 2), (q - 1, ds[0]), (2, 1 << l),
                                              (0, 5), (q, 5)]):
                    h = hq[i % 4]
                    dbytes, kbytes = dd.to_bytes(no, "little"), kk.to_bytes(no, "little")
                    sig = ctypes.create_string_buffer(no + no // 2)
                    code = L.bignSign(sig, ctypes.byref(prm), oid, _sz(len(oid)), h, dbytes, MS.replay(kbytes), None) & 0xFFFFFFFF
                    assert (code, sig.raw if code == 0 else b"") == OG.sign_k(P, oid, h, dbytes, kbytes, ref_belt_hash), (l, i)
                    out["sign_k"].append({"set": si, "by": "reference", "oid": oid.hex(), "hash": h.hex(), "priv": dbytes.hex(), "k": kbytes.hex(),
                                          "code": code, "sig": sig.raw.hex() if code == 0 else ""})
            elif kind == "adv":
                for dd, kk, h in ((rnd.randrange(1, q), rnd.randrange(1, q), rnd.randbytes(no)),
                                  (q - 1, q - 1, ((1 << (2 * l)) - 1).to_bytes(no, "little"))):
                    dbytes, kbytes = dd.to_bytes(no, "little"), kk.to_bytes(no, "little")
                    code, pk = OG.pubkey_calc(P, dbytes)
                    out["pubkey_calc"].append({"set": si, "by": "python", "priv": dbytes.hex(), "code": code, "pub": pk.hex()})
                    code, sig = OG.sign_k(P, oid, h, dbytes, kbytes, ref_belt_hash)
                    out["sign_k"].append({"set": si, "by": "python", "oid": oid.hex(), "hash": h.hex(), "priv": dbytes.hex(), "k": kbytes.hex(),
                                          "code": code, "sig": sig.hex()})
        print("l =", l, "done:", len(out["sets"]), "sets so far")
    path = os.path.join(ROOT, "tests", "golden", "bign_generic_adv.json")
    json.dump(out, open(path, "w"), indent=0)
    from collections import Counter
    print({k: len(v) for k, v in out.items()}, Counter(c["code"] for c in out["verify"]),
          Counter((c["name"], c["code"]) for c in out["crafted"]), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
