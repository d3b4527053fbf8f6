#!/usr/bin/env python3
"""tests/golden/bign_sign_tail.json: signatures on the three standard curves whose PRIVATE KEY is steered so that the tail of
signing, s1 = (k - (s0 + 2^l) d - H) mod q, takes the branches that random inputs reach with probability near 2^-128
(tests/signtail.py reads the file and restates the tail in integers).  Build container only: every signature is the reference's
bignSign with a generator that replays k, every public key its bignPubkeyCalc, every verdict its bignVerify
(oracle/_ref/libbee2ref.so through tools/refgen.py).

How d is steered: s0 = belt-hash(oid || x(k G) || H) does not depend on d.  Choose k, H and the OID, read s0 off a signature made
under the throw-away key d = 1, set d = r / (s0 + 2^l) mod q: under that key (s0 + 2^l) d = r (mod q).  The second signature
must carry the same s0 or the tool stops.

Per level a record {l, kind, name, oid, priv, k, hash, sig, pub, verify}; r = (s0 + 2^l) d mod q, u = (k - r) mod q, W = 2^(2l),
cq = W - q; the OID alternates between the level's own and one of another length mod 4 (tests/golden/bign_oid_lengths.json):
  fold  r = 1, 2, cq - 1 (mod_q_ct's final subtraction taken), cq, cq + 1, q - 2, q - 1 (not taken); r = 2 with k = 1 and r = cq - 1
        with k = cq - 2 (taken, and k < r: with k >= r the borrow of k - r would hide a subtraction that was left out); one record for every
        event (top, t2, sub) of signtail.reachable(l, q) -- the top limb after the first fold, the one the second small pass meets,
        the final subtraction -- found by a seeded search: k fixed, H and r (inside the event's range of r) drawn until the
        model of the fold names that event.  On the 384-bit curve the first fold reaches 4 q, so t2 = 1 occurs, with top 1, 2, 3.
  sub1  u = 0 (r = k), u = q - 1 (r = k + 1), u = 1, k = 1 with r = q - 1, k = q - 1 with r = 1.
  sub2  H < q: s1 = 0 (H = u), s1 = q - 1 (H = u + 1), s1 = 1, H = 0, H = q - 1 with u = 0.
  hge   H >= q and u >= H - q, s1 still a residue: H = q with u = 0; H = q + c with u = c and u = c + 1; H = W - 1 with u = cq - 1
        and u = cq.
  wrap  H >= q and u < H - q: the reference's zzSubMod is handed the raw H (bign_sign.c:236-238) and what it writes is NOT below
        q: H = W - 1 with u = 0 and u = cq - 2, H = q + 1 with u = 0.  sig is whatever the reference wrote, verify whatever it
        answers to that (ERR_BAD_SIG: s1 >= q)."""
import ctypes
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import refgen  # noqa: E402
import make_golden_sign as MS  # noqa: E402
import signtail as T  # noqa: E402

_sz = ctypes.c_size_t
SEED = 0x7A11
SEARCH_CAP = 1 << 17
OTHER_OID_RESIDUE = {128: 0, 192: 1, 256: 2}        # the level's own OID has 11 octets


def belt_hash(m):
    out = ctypes.create_string_buffer(32)
    assert refgen.ref().beltHash(out, m, _sz(len(m))) == 0
    return out.raw


def other_oid(l):
    for x in json.load(open(os.path.join(ROOT, "tests", "golden", "bign_oid_lengths.json"))):
        o = bytes.fromhex(x["oid"])
        if len(o) % 4 == OTHER_OID_RESIDUE[l]:
            return o
    raise SystemExit("no OID of that length")


class Level:
    def __init__(self, l):
        self.l, self.no = l, l // 4
        self.P = MS.params(l)
        self.q = T.le(bytes(self.P.q)[:self.no])
        assert self.q == T.curve_q(l)
        self.W = 1 << (2 * l)
        self.cq = self.W - self.q
        self.oids = (MS.OID[l], other_oid(l))
        assert len(self.oids[0]) % 4 != len(self.oids[1]) % 4

    def enc(self, x):
        return x.to_bytes(self.no, "little")

    def sign(self, oid, H, d, k):
        code, sig, used = MS.r_sign(self.l, oid, self.enc(H), self.enc(d), self.enc(k))
        assert code == 0 and used == self.no, (code, used)
        return sig

    def pub(self, d):
        code, pub = MS.r_pubkey_calc(self.l, self.enc(d))
        assert code == 0
        return pub

    def verify(self, oid, H, sig, pub):
        return refgen.ref().bignVerify(ctypes.byref(self.P), oid, _sz(len(oid)), self.enc(H), sig, pub) & 0xFFFFFFFF

    def s0(self, oid, xR, H):
        """as bign_sign.c:226-231 -- for the searches only; a record's s0 is read off the reference's signature"""
        return T.le(belt_hash(oid + xR + self.enc(H))[:self.l // 8])

    def key_for(self, s0, r):
        return r * pow(s0 + (1 << self.l), -1, self.q) % self.q


# ---- the plans: (name, k, H, r) per kind; the searched events of the fold are the only ones that need the reference
def plan_fold(Lv, rnd, oid_of):
    q, cq = Lv.q, Lv.cq
    out = [(name, rnd.randrange(1, q), rnd.randrange(q), r) for name, r in
           (("r=1", 1), ("r=2", 2), ("r=cq-1", cq - 1), ("r=cq", cq), ("r=cq+1", cq + 1), ("r=q-2", q - 2), ("r=q-1", q - 1))]
    # the final subtraction taken AND k < r: were q not taken off, k - (r + q) would borrow, + q, and leave k - r + W, no residue
    # (with k >= r the second step hides it: k - (r + q) + q = k - r all the same)
    out += [("r=2 k=1", 1, rnd.randrange(q), 2), ("r=cq-1 k=cq-2", cq - 2, rnd.randrange(q), cq - 1)]
    for event, (lo, hi) in sorted(T.reachable(Lv.l, q).items()):
        oid = oid_of(len(out))
        k = rnd.randrange(1, q)
        xR = Lv.pub(k)[:Lv.no]
        for tries in range(1, SEARCH_CAP + 1):
            H, r = rnd.randrange(q), rnd.randrange(lo, hi + 1)
            s0 = Lv.s0(oid, xR, H)
            if T.fold_events(Lv.l, q, T.product(Lv.l, s0, Lv.key_for(s0, r)))[0] == event:
                break
        else:
            raise SystemExit(f"l = {Lv.l}, event {event}: nothing in {SEARCH_CAP} tries")
        out.append(("top=%d t2=%d sub=%d" % event, k, H, r))
    return out


PLANS = {"fold": plan_fold, "sub1": lambda Lv, rnd, oid_of: T.plan_sub1(Lv.l, Lv.q, rnd), "sub2": lambda Lv, rnd, oid_of: T.plan_sub2(Lv.l, Lv.q, rnd),
         "hge": lambda Lv, rnd, oid_of: T.plan_hge(Lv.l, Lv.q, rnd), "wrap": lambda Lv, rnd, oid_of: T.plan_wrap(Lv.l, Lv.q, rnd)}


def realise(Lv, kind, name, oid, k, H, r):
    """the two signatures of the steering -> a record"""
    l, q = Lv.l, Lv.q
    assert 0 < k < q and 0 < r < q and 0 <= H < Lv.W
    s0 = Lv.sign(oid, H, 1, k)[:l // 8]
    d = Lv.key_for(T.le(s0), r)
    sig = Lv.sign(oid, H, d, k)
    if sig[:l // 8] != s0:
        raise SystemExit(f"l = {l}, {kind} {name}: s0 moved with the private key")
    pub = Lv.pub(d)
    t = T.tail(l, q, T.le(s0), d, k, H)
    assert t["r"] == r and T.le(sig[l // 8:]) == t["s1"], (l, kind, name, "the model of the tail disagrees with the reference")
    return {"l": l, "kind": kind, "name": name, "oid": oid.hex(), "priv": Lv.enc(d).hex(), "k": Lv.enc(k).hex(), "hash": Lv.enc(H).hex(),
            "sig": sig.hex(), "pub": pub.hex(), "verify": Lv.verify(oid, H, sig, pub)}


def level_records(l, rnd, kinds=T.KINDS):
    """every kind's records of one level, the OID alternating inside each kind"""
    Lv = Level(l)
    out = []
    for kind in kinds:
        oid_of = lambda i: Lv.oids[i % 2]
        for i, (name, k, H, r) in enumerate(PLANS[kind](Lv, rnd, oid_of)):
            out.append(realise(Lv, kind, name, oid_of(i), k, H, r))
    return out


def build(seed=SEED):
    rnd = random.Random(seed)
    return [r for l in T.LEVELS for r in level_records(l, rnd)]


def main(path=T.PATH):
    recs = build()
    for r in recs:
        assert (r["verify"] == T.ERR_BAD_SIG) == (r["kind"] == "wrap") and r["verify"] in (0, T.ERR_BAD_SIG), (r["l"], r["kind"], r["name"], r["verify"])
    lines = ['{"records":['] + [json.dumps(r, separators=(",", ":")) + ("," if i + 1 < len(recs) else "") for i, r in enumerate(recs)] + ["]}"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    json.load(open(path))
    from collections import Counter
    for l in T.LEVELS:
        print("l =", l, dict(Counter(r["kind"] for r in recs if r["l"] == l)))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if not refgen.have_ref():
        raise SystemExit("oracle/_ref/libbee2ref.so missing: run `make -C oracle ref` in the build container")
    main()
