#!/usr/bin/env python3
"""tests/golden/bign_sign2_nonce.json -- the one-time key of bignSign2 (STB 34.101.45 algorithm 6.3.3) on parameter sets
whose q REJECTS draws: every non-"iso" set of tests/golden/bign_generic_adv.json (referred to by index) and the "iso" set
of each level.  Build container only: every signature is the reference's bignSign2 (oracle/_ref/libbee2ref.so).

Per record {set, oid, priv, t, hash, k, passes, sig, code}:
  * k is recovered from the reference's signature, k = s1 + (s0 + 2^l) d + H mod q.  That holds whatever R was: on a set
    whose q is not the group order the reference's R is an artefact of its scalar recoding (tools/make_golden_generic_sign.py),
    but s1 is computed from k, s0 and d all the same (bign_sign.c:231-239).
  * H is drawn BELOW q.  The reference's tail subtracts H from a residue with zzSubMod (bign_sign.c:237-239), which takes
    operands below q; with H >= q the result leaves [0, q) whenever the residue is below H - q.  On the standard curves
    2^(2l) - q is tiny and that never shows; on q = 2^(2l-1) + 1 about a quarter of such records would carry an s1 that is no
    residue at all.  That is the reference's tail, not its one-time key, so the pin stays where both are defined.
  * k is made a second time by driving the reference's beltHash / beltWBLStart / beltWBLStepE exactly as bign_sign.c:195-217
    does -- ONE state, beltWBLStepE again and again -- and a third time by the model (tests/orc_sign2.py) on the reference's
    primitives, each pass a fresh belt-wbl.  All three have to agree or the tool stops: beltWBLStepE starts its round counter
    anew on every call (belt_wbl.c:203).  "passes" is the count the replay needed.
  * d is in range (1 and q - 1 among them), t runs over none, 1, 31, 32, 33, 64, 65, 200 octets, the OID over lengths
    0..3 mod 4 (from tests/golden/bign_oid_lengths.json).
  * on the q = 2^(2l-1) + 1 sets the seeded inputs are searched so that, per level, pass counts 1, 2, 3, 4 and one >= 6 occur.
On the "iso" sets the model's whole bignSign2 must equal the reference's signature too."""
import ctypes
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import refgen  # noqa: E402
import orc_generic as OG  # noqa: E402
import orc_sign2 as S2  # noqa: E402
from make_golden_generic import ref_belt_hash  # noqa: E402
from make_golden_generic_sign import mkparams  # noqa: E402

L = refgen.ref()
_sz = ctypes.c_size_t
L.beltWBL_keep.restype = _sz
T_LENS = (None, 1, 31, 32, 33, 64, 65, 200)
PER_SET = 12
TARGETS = (1, 2, 3, 4, 6)            # records 0..4 of a q = 2^(2l-1) + 1 set: that many passes (the last: at least)


def ref_wbl(msg, key):
    """one belt-wbl encryption on a fresh state"""
    st = ctypes.create_string_buffer(L.beltWBL_keep())
    L.beltWBLStart(st, bytes(key), _sz(len(key)))
    buf = ctypes.create_string_buffer(bytes(msg), len(msg))
    L.beltWBLStepE(buf, _sz(len(msg)), st)
    return 0, buf.raw


def ref_replay(oid, d, t, h, q):
    """bign_sign.c:195-217 on the reference's own primitives: (k, passes)"""
    theta = ref_belt_hash(oid + d + (t or b""))
    st = ctypes.create_string_buffer(L.beltWBL_keep())
    L.beltWBLStart(st, theta, _sz(32))
    buf = ctypes.create_string_buffer(bytes(h), len(h))
    passes = 0
    while True:
        L.beltWBLStepE(buf, _sz(len(h)), st)
        passes += 1
        if 0 < OG.le(buf.raw) < q:
            return OG.le(buf.raw), passes


def oids_by_residue():
    seen = {}
    for x in json.load(open(os.path.join(ROOT, "tests", "golden", "bign_oid_lengths.json"))):
        o = bytes.fromhex(x["oid"])
        seen.setdefault(len(o) % 4, o)
    assert sorted(seen) == [0, 1, 2, 3]
    return [seen[r] for r in range(4)]


def build():
    """the fixture as a dict, and the pass counts per (l, kind of q)"""
    rnd = random.Random(0x6E6F6E63)
    A = json.load(open(os.path.join(ROOT, "tests", "golden", "bign_generic_adv.json")))
    oids = oids_by_residue()
    out = {"oids": [o.hex() for o in oids], "records": []}
    hist = {}
    for si, s in enumerate(A["sets"]):
        prm, P = mkparams(s), OG.Params.from_hex(s)
        l = s["l"]
        no = l // 4
        q = OG.le(bytes.fromhex(s["q"]))
        enc = lambda v: v.to_bytes(no, "little")
        for j in range(PER_SET):
            oid = oids[(j + si) % 4]
            tl = T_LENS[j % 8]
            want = TARGETS[j] if s["q_kind"] == "2^(2l-1) + 1" and j < len(TARGETS) else None
            while True:
                d = enc(1 if j == 10 else q - 1 if j == 11 else rnd.randrange(1, q))
                h = enc(q - 1 if j == 9 else 0 if j == 8 else rnd.randrange(q))
                t = None if tl is None else rnd.randbytes(tl)
                k, passes = ref_replay(oid, d, t, h, q)
                if want is None or passes == want or (want == 6 and passes >= 6):
                    break
            sig = ctypes.create_string_buffer(no + no // 2)
            code = L.bignSign2(sig, ctypes.byref(prm), oid, _sz(len(oid)), h, d, t, _sz(len(t) if t else 0)) & 0xFFFFFFFF
            assert code == 0, (si, j, code)
            assert S2.recover_k(l, q, sig.raw, d, h) == k, (si, j, "the reference's signature holds another k than the replay")
            assert S2.nonce(oid, d, t, h, q, ref_belt_hash, ref_wbl) == (k, passes), (si, j, "model")
            if s["kind"] == "iso":
                assert S2.sign2(P, oid, h, d, t, ref_belt_hash, ref_wbl) == (0, sig.raw), (si, j)
            out["records"].append({"set": si, "oid": oid.hex(), "priv": d.hex(), "t": None if t is None else t.hex(), "hash": h.hex(),
                                   "k": enc(k).hex(), "passes": passes, "sig": sig.raw.hex(), "code": code})
            hist.setdefault((l, s["q_kind"]), []).append(passes)
    for l in (128, 192, 256):
        got = hist[(l, "2^(2l-1) + 1")]
        assert {1, 2, 3, 4} <= set(got) and max(got) >= 6, (l, got)
    return out, hist


def main():
    out, hist = build()
    path = os.path.join(ROOT, "tests", "golden", "bign_sign2_nonce.json")
    json.dump(out, open(path, "w"), indent=0)
    for key, v in sorted(hist.items()):
        print(key, sorted(v))
    print(len(out["records"]), "records,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
