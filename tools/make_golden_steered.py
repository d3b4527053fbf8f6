#!/usr/bin/env python3
"""tests/golden/bign_steered.json: signatures on the three standard curves whose verification scalars are STEERED, for the walks
of R = u G + v Q in bee2_amd/csrc/bign_kernels.hip and host_bign.hpp (u = (s1 + H) mod q, v = s0 + 2^l; tests/steered.py reads the
file and models the walk).  Build container only: every signature and public key is made by the reference (oracle/_ref/libbee2ref.so:
bignSign with a generator that replays k, bignPubkeyCalc), every expected code is the reference's bignVerify, and each record is
cross-checked with the oracle (orc.verify_batch_l) before the file is written.

How u is steered: s0 = belt-hash(oid || x(k G) || H) does not depend on the private key.  For a wanted U choose k and H, read s0 off
a signature made with that k, set d = (k - U) / (s0 + 2^l) mod q: the genuine signature of H under Q = d G with that k has u = U.

Families, per l in {128, 192, 256}, nw = l / 8 comb windows of 16 bits:
  a  extremes of u: 0, 1, 2, q - 1, q - 2; 2^(16 j) for every j; 0xFFFF 2^(16 j) for j = 0, nw / 2 and the highest j below q.
  b  zero windows of u, the others seeded-random and non-zero: exactly window j, for every j; the lowest half, the highest half;
     every j = r (mod 4), r = 0..3 (a lane of bign_onekey4_kernel with no window of u); only j = r (mod 4), r = 0..3.
  c  windows of v under ONE key per curve (d fixed, not kept): with k fixed, x(k G) is too, and H is ground over a seeded sequence
     until s0 has octet 0 / the middle octet / the last octet zero (an empty 8-bit window), 16-bit word 0 / the last word zero (an
     empty window of the 16-bit key table), the top octet 0xFF, then 0x00; at most 2^20 tries each.  The signature is the
     reference's, with that k.  The signer comes with a pool of ordinary signatures.
  d  exceptional steps of the serial walk (T = v Q, then the windows of u in ascending order), S_j = sum_{w<j} u_w 2^(16 w): for
     eps = +-1 and j in {0, nw / 2, nw - 1}, U with every window non-zero, D = eps u_j 2^(16 j) - S_j, k = U + D, d = D / v: before
     window j the accumulator is eps times the comb point it is about to add (eps = +1 a doubling, eps = -1 the sum is O); and the
     final fold D = U, k = 2 U, v Q == u G.  These keys are throw-away: d is kept, for the model.
     eps = -1 at j = nw - 1 makes k = U + D = 0: R = O, which no signer produces.  That record is built by hand (s0 seeded-random,
     s1 = U - H, the key from the reference's bignPubkeyCalc) and is NOT a valid signature: the reference says ERR_BAD_SIG.
  e  neighbours that must fail: for every case of b, s1' = s1 + 2^(16 j) mod q for its lowest and its highest zero window j (where
     they are one window, the second neighbour adds 0xFFFF 2^(16 j)); for U = 0, s1' = s1 + 1.  Same hash and key; stored with
     the signature only.
Not here: collisions between the partial sums of the lanes in the quad fold (circular: the model would be the kernel), and a lane of
bign_onekey4_kernel with no window of v either (a 32-bit grind of s0: out of budget)."""
import ctypes
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import refgen  # noqa: E402
import make_golden_sign as MS  # noqa: E402
import steered as ST  # noqa: E402

_sz = ctypes.c_size_t
POOL = 10
GRIND_CAP = 1 << 20


def belt_hash(m):
    out = ctypes.create_string_buffer(32)
    assert refgen.ref().beltHash(out, m, _sz(len(m))) == 0
    return out.raw


class Curve:
    def __init__(self, l):
        self.l, self.no, self.oid = l, l // 4, MS.OID[l]
        self.P = MS.params(l)
        self.q = ST.le(bytes(self.P.q)[:self.no])
        self.nw = ST.nw(l)

    def le(self, x):
        return MS.le(x, self.no)

    def sign(self, h, d, k):
        code, sig, used = MS.r_sign(self.l, self.oid, h, self.le(d), self.le(k))
        assert code == 0 and used == self.no, (code, used)
        return sig

    def pub(self, d):
        code, pub = MS.r_pubkey_calc(self.l, self.le(d))
        assert code == 0
        return pub

    def verify(self, h, sig, pub):
        return refgen.ref().bignVerify(ctypes.byref(self.P), self.oid, _sz(len(self.oid)), h, sig, pub) & 0xFFFFFFFF

    def steer(self, rnd, U, k=None, D=None):
        """a genuine (hash, sig, pubkey, d) with u = U; k given: with that one-time key and v d = D"""
        q = self.q
        h = rnd.randbytes(self.no)
        if k is None:
            k = rnd.randrange(1, q)
            while k == U:
                k = rnd.randrange(1, q)
            D = (k - U) % q
        assert 0 < k < q and D % q and (U + D) % q == k
        s0 = self.sign(h, 1, k)[:self.no // 2]
        d = D * pow(ST.le(s0) + (1 << self.l), -1, q) % q
        sig = self.sign(h, d, k)
        assert sig[:self.no // 2] == s0 and ST.u_of(self.l, q, h, sig) == U
        return h, sig, self.pub(d), d

    def random_windows(self, rnd, zero):
        """U < q with the windows in `zero` zero and the others non-zero"""
        while True:
            U = ST.from_windows16([0 if j in zero else rnd.randrange(1, 1 << 16) for j in range(self.nw)])
            if U < self.q:
                return U


def family_a(C, rnd):
    q, nw = C.q, C.nw
    top = max(j for j in range(nw) if 0xFFFF << (16 * j) < q)
    targets = [("u=0", 0), ("u=1", 1), ("u=2", 2), ("u=q-1", q - 1), ("u=q-2", q - 2)]
    targets += [(f"u=1<<16*{j}", 1 << (16 * j)) for j in range(nw)]
    targets += [(f"u=ffff<<16*{j}", 0xFFFF << (16 * j)) for j in (0, nw // 2, top)]
    return [(name, U) + C.steer(rnd, U) for name, U in targets]


def family_b(C, rnd):
    nw = C.nw
    sets = [(f"zero w{j}", {j}) for j in range(nw)]
    sets += [("zero low half", set(range(nw // 2))), ("zero high half", set(range(nw // 2, nw)))]
    sets += [(f"zero j%4=={r}", {j for j in range(nw) if j % 4 == r}) for r in range(4)]
    sets += [(f"only j%4=={r}", {j for j in range(nw) if j % 4 != r}) for r in range(4)]
    out = []
    for name, zero in sets:
        U = C.random_windows(rnd, zero)
        assert {j for j, w in enumerate(ST.windows16(U, C.l)) if w == 0} == zero
        out.append((name, U) + C.steer(rnd, U) + (sorted(zero),))
    return out


def family_c(C, rnd):
    """-> (cases, signer): one key, s0 ground over the hashes"""
    q, no = C.q, C.no
    d = rnd.randrange(1, q)
    pub = C.pub(d)
    half = no // 2
    goals = [("s0 octet 0 zero", lambda s: s[0] == 0), (f"s0 octet {half // 2} zero", lambda s: s[half // 2] == 0),
             (f"s0 octet {half - 1} zero", lambda s: s[half - 1] == 0), ("s0 word 0 zero", lambda s: s[0] == 0 and s[1] == 0),
             (f"s0 word {half // 2 - 1} zero", lambda s: s[half - 2] == 0 and s[half - 1] == 0),
             ("s0 top octet ff", lambda s: s[half - 1] == 0xFF), ("s0 top octet 00", lambda s: s[half - 1] == 0)]
    cases = []
    for name, goal in goals:
        k = rnd.randrange(1, q)
        xR = C.pub(k)[:no]
        hrnd = random.Random(rnd.getrandbits(64))
        for tries in range(1, GRIND_CAP + 1):
            h = hrnd.randbytes(no)
            if goal(belt_hash(C.oid + xR + h)[:half]):
                break
        else:
            raise SystemExit(f"l = {C.l}, {name}: nothing in 2^20 tries")
        sig = C.sign(h, d, k)
        assert goal(sig[:half]), name
        print(f"  l = {C.l}  c  {name}: {tries} tries")
        cases.append((name, ST.u_of(C.l, q, h, sig), h, sig, pub, None))
    pool = []
    for _ in range(POOL):
        h = rnd.randbytes(no)
        pool.append((h, C.sign(h, d, rnd.randrange(1, q))))
    return cases, {"pubkey": pub, "pool": pool}


def family_d(C, rnd):
    q, nw, l, no = C.q, C.nw, C.l, C.no
    out = []
    for eps, kind in ((1, "E"), (-1, "-E")):
        for j in (0, nw // 2, nw - 1):
            U = C.random_windows(rnd, set())
            ws = ST.windows16(U, l)
            S = ST.from_windows16(ws[:j])
            D = (eps * (ws[j] << (16 * j)) - S) % q
            k = (U + D) % q
            name = f"{kind} at w{j}"
            if k == 0:                                   # eps = -1 at the top window: R = O, not a signature anyone can make
                assert (eps, j) == (-1, nw - 1)
                h = rnd.randbytes(no)
                s0 = rnd.randbytes(no // 2)
                d = D * pow(ST.le(s0) + (1 << l), -1, q) % q
                H = ST.le(h) - q if ST.le(h) >= q else ST.le(h)
                sig = s0 + C.le((U - H) % q)
                rec = (h, sig, C.pub(d), d)
                assert ST.u_of(l, q, h, sig) == U
            else:
                rec = C.steer(rnd, U, k, D)
            h, sig, pub, d = rec
            ev = ST.walk(l, q, U, ST.v_of(l, sig), d)
            assert ev and ev[0] == (j, kind), (name, ev)
            out.append((name, U) + rec)
    U = C.random_windows(rnd, set())
    while 2 * U % q == 0:
        U = C.random_windows(rnd, set())
    rec = C.steer(rnd, U, 2 * U % q, U)
    assert ST.fold(q, U, ST.v_of(l, rec[1]), rec[3]) == "E" and not ST.walk(l, q, U, ST.v_of(l, rec[1]), rec[3])
    out.append(("fold E", U) + rec)
    return out


def family_e(C, a, b):
    q, no = C.q, C.no
    out = []

    def bump(name, U, h, sig, delta, j):
        s1 = (ST.le(sig[no // 2:]) + delta) % q
        s = sig[:no // 2] + C.le(s1)
        assert ST.u_of(C.l, q, h, s) == (U + delta) % q
        return (name, (U + delta) % q, s, j)
    for name, U, h, sig, pub, d, zero in b:
        lo, hi = zero[0], zero[-1]
        out.append((name,) + bump(f"{name} +1<<16*{lo}", U, h, sig, 1 << (16 * lo), lo))
        if hi != lo:
            out.append((name,) + bump(f"{name} +1<<16*{hi}", U, h, sig, 1 << (16 * hi), hi))
        else:
            out.append((name,) + bump(f"{name} +ffff<<16*{lo}", U, h, sig, 0xFFFF << (16 * lo), lo))
    name, U, h, sig, pub, d = a[0]
    assert U == 0
    out.append((name,) + bump("u=0 +1", U, h, sig, 1, 0))
    return out


def main(path=ST.PATH):
    import orclib
    orc = orclib.load()
    rnd = random.Random(0x57EE12ED)
    lines = ['{"q":{' + ",".join(f'"{l}":"{Curve(l).q:x}"' for l in ST.LEVELS) + '},', '"curves":{']
    for l in ST.LEVELS:
        C = Curve(l)
        a, b = family_a(C, rnd), family_b(C, rnd)
        c, csigner = family_c(C, rnd)
        d = family_d(C, rnd)
        e = family_e(C, a, b)
        signers = [csigner] + [{"pubkey": r[4], "d": r[5], "pool": []} for r in d]
        recs, full = [], []

        def put(family, name, U, h, sig, pub, extra, parent=None):
            code = C.verify(h, sig, pub)
            r = {"family": family, "name": name, "U": f"{U:x}", "code": code}
            if parent is None:
                r.update(hash=h.hex(), pubkey=pub.hex())
            else:
                r["parent"] = parent
            r["sig"] = sig.hex()
            r.update(extra)
            recs.append(r)
            full.append((h, sig, pub, code, family, name))
        for name, U, h, sig, pub, dd in a:
            put("a", name, U, h, sig, pub, {})
        by = {}
        for name, U, h, sig, pub, dd, zero in b:
            put("b", name, U, h, sig, pub, {})
            by[name] = (h, pub)
        by[a[0][0]] = (a[0][2], a[0][4])
        for name, U, h, sig, pub, dd in c:
            put("c", name, U, h, sig, pub, {"key_index": 0})
        for i, (name, U, h, sig, pub, dd) in enumerate(d):
            put("d", name, U, h, sig, pub, {"key_index": 1 + i, "d": f"{dd:x}"})
        for parent, name, U, sig, j in e:
            put("e", name, U, by[parent][0], sig, by[parent][1], {"window": j}, parent=parent)
        # what the families promise, in the reference's own verdicts
        for h, sig, pub, code, family, name in full:
            want = ST.ERR_BAD_SIG if family == "e" or name == f"-E at w{C.nw - 1}" else 0
            assert code == want, (l, family, name, code)
        for h, sig in csigner["pool"]:
            assert C.verify(h, sig, csigner["pubkey"]) == 0
        got = orc.verify_batch_l(l, C.oid, b"".join(x[0] for x in full), b"".join(x[1] for x in full), b"".join(x[2] for x in full))
        assert got == [x[3] for x in full], (l, [(x[5], g) for x, g in zip(full, got) if g != x[3]])
        lines.append(f'"{l}":{{"cases":[')
        lines += [json.dumps(r, separators=(",", ":")) + ("," if i + 1 < len(recs) else "") for i, r in enumerate(recs)]
        lines.append('],"signers":[')
        for i, s in enumerate(signers):
            r = {"pubkey": s["pubkey"].hex(), "pool": [[h.hex(), g.hex()] for h, g in s["pool"]]}
            if "d" in s:
                r["d"] = f"{s['d']:x}"
            lines.append(json.dumps(r, separators=(",", ":")) + ("," if i + 1 < len(signers) else ""))
        lines.append("]}" + ("," if l != ST.LEVELS[-1] else ""))
        from collections import Counter
        print("l =", l, dict(Counter(r["family"] for r in recs)), dict(Counter(r["code"] for r in recs)))
    lines.append("}}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    json.load(open(path))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if not refgen.have_ref():
        raise SystemExit("oracle/_ref/libbee2ref.so missing: run `make -C oracle ref` in the build container")
    main()
