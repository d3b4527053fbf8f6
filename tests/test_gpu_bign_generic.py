"""GPU: bignVerify / bignPubkeyVal on NON-STANDARD parameter sets (bign_generic_kernels.hip) against the fixtures the
reference produced (tests/golden/bign_generic.json) and against the Python restatement (tests/orc_generic.py) on
fresh random damage."""
import ctypes
import json
import os
import random

import pytest

import orc_generic as OG
import orc_sign2 as S2
from bee2_amd.engine import bign_params
from gpulib import engine

pytestmark = pytest.mark.gpu

FIX = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bign_generic.json")))


def mk(c):
    prm = bign_params()
    prm.l = c["l"]
    for f in ("p", "a", "b", "q", "yG"):
        raw = bytes.fromhex(c[f])
        ctypes.memmove(getattr(prm, f), raw + bytes(64 - len(raw)), 64)
    return prm


def test_generic_verify_batches_match_the_reference():
    """every case of a curve in ONE bee2hip_bignVerify_batch call: valid signatures on isomorphic images of the standard
    curves (reference as signer) and on random-prime curves (no-wrap signatures the reference accepts), damaged variants"""
    eng = engine()
    for ci, c in enumerate(FIX["curves"]):
        prm = mk(c)
        cases = [x for x in FIX["cases"] if x["curve"] == ci]
        H = b"".join(bytes.fromhex(x["hash"]) for x in cases)
        S = b"".join(bytes.fromhex(x["sig"]) for x in cases)
        K = b"".join(bytes.fromhex(x["pubkey"]) for x in cases)
        code, got = eng.bignVerify_batch(H, S, K, oid_der=bytes.fromhex(cases[0]["oid"]), params=prm)
        assert code == 0, (ci, code)
        bad = [(x["name"], g, x["code"]) for x, g in zip(cases, got) if g != x["code"]]
        assert not bad, (ci, c["kind"], c["l"], bad[:5])
        assert 0 in got and 510 in got


def test_generic_verify_dropin_and_pubkey_val():
    eng = engine()
    for ci, c in enumerate(FIX["curves"]):
        prm = mk(c)
        cases = [x for x in FIX["cases"] if x["curve"] == ci][:3]
        for x in cases:
            got = eng.bignVerify(prm, bytes.fromhex(x["oid"]), bytes.fromhex(x["hash"]), bytes.fromhex(x["sig"]), bytes.fromhex(x["pubkey"]))
            assert got == x["code"], (ci, x["name"], got)
        pv = [x for x in FIX["pubkey_val"] if x["curve"] == ci]
        code, got = eng.bignPubkeyVal_batch(b"".join(bytes.fromhex(x["pubkey"]) for x in pv), prm)
        assert code == 0 and got == [x["code"] for x in pv], (ci, got)
        assert eng.bignPubkeyVal(prm, bytes.fromhex(pv[0]["pubkey"])) == pv[0]["code"]


def test_malformed_parameter_sets_report_the_reference_codes():
    eng = engine()
    for c in FIX["bad_params"]:
        prm = mk(c)
        h, s, k = (bytes.fromhex(c[x]) for x in ("hash", "sig", "pubkey"))
        assert eng.bignVerify(prm, bytes.fromhex(c["oid"]), h, s, k) == c["verify"], c["name"]
        assert eng.bignPubkeyVal(prm, k) == c["pubkey_val"], c["name"]
        # precedence as bignVerify: parameters (incl. what bignEcCreate rejects), then inputs, then the OID
        codes = (ctypes.c_uint32 * 1)()
        code = eng.lib.bee2hip_bignVerify_batch(ctypes.byref(prm), b"\x06\x01", ctypes.c_size_t(2), h, s, k, ctypes.c_size_t(1), codes)
        assert code == (c["verify"] if c["verify"] not in (0, 505, 510) else 301), c["name"]     # 301 = ERR_BAD_OID


def test_generic_verify_random_damage_vs_python_restatement(orc):
    """fresh corruptions of the fixture triples (the fixtures fix only a few): the Python restatement, pinned to the
    reference by tests/test_oracle_golden.py, is the checker"""
    eng = engine()
    rnd = random.Random(0x67656E)
    for ci, c in enumerate(FIX["curves"]):
        if c["l"] == 256 and c["kind"] == "rnd":
            continue                                            # the Python checker needs ~0.3 s per 512-bit case
        prm = mk(c)
        P = OG.Params.from_hex(c)
        no = c["l"] // 4
        good = [x for x in FIX["cases"] if x["curve"] == ci and x["name"] == "good"]
        H, S, K, want = b"", b"", b"", []
        for _ in range(12):
            x = rnd.choice(good)
            h, s, k = (bytearray.fromhex(x[f]) for f in ("hash", "sig", "pubkey"))
            r = rnd.randrange(5)
            if r == 1:
                s[rnd.randrange(len(s))] ^= 1 << rnd.randrange(8)
            elif r == 2:
                h[rnd.randrange(no)] ^= 1 << rnd.randrange(8)
            elif r == 3:
                k[rnd.randrange(2 * no)] ^= 1 << rnd.randrange(8)
            elif r == 4:
                s[no // 2:] = rnd.getrandbits(8 * no).to_bytes(no, "little")
            H += bytes(h); S += bytes(s); K += bytes(k)
            want.append(OG.verify(P, bytes.fromhex(x["oid"]), bytes(h), bytes(s), bytes(k), orc.belt_hash))
        code, got = eng.bignVerify_batch(H, S, K, oid_der=bytes.fromhex(good[0]["oid"]), params=prm)
        assert code == 0 and got == want, (ci, got, want)


SFIX = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bign_generic_sign.json")))


@pytest.mark.parametrize("which", range(len(SFIX)))
def test_generic_signing_side_matches_the_reference(which):
    """round 3: bignPubkeyCalc / bignKeypairGen / bignSign2 / bignSign on isomorphic images of the standard curves (a != -3;
    the constant-time general-curve ladder of bign_generic_kernels.hip) -- keys 0, 1, q - 1, q, 2^2l - 1, hashes at and beyond
    q, additional input up to 200 octets (the host-hashed theta path), a 203-octet OID, rejected rng draws, a malformed OID;
    every expected value from the reference (tools/make_golden_generic_sign.py).  What is signed here must also verify here."""
    eng = engine()
    ent = SFIX[which]
    c = FIX["curves"][ent["curve"]]
    P = mk(c)
    no = c["l"] // 4
    for x in ent["pubkey_calc"]:
        code, pub = eng.bignPubkeyCalc(P, bytes.fromhex(x["priv"]))
        assert code == x["code"], x["priv"]
        if code == 0:
            assert pub.hex() == x["pub"]
            assert eng.bignPubkeyVal(P, pub) == 0
    for x in ent["keypair_gen"]:
        rng = eng.rng_from_bytes(bytes.fromhex(x["rnd"]) + bytes(70 * no))
        code, priv, pub = eng.bignKeypairGen(P, rng)
        assert code == x["code"], x
        if code == 0:
            assert (priv.hex(), pub.hex(), rng.pos[0]) == (x["priv"], x["pub"], x["used"])
    for x in ent["sign2"]:
        t = None if x["t"] is None else bytes.fromhex(x["t"])
        oid, h, d = (bytes.fromhex(x[k]) for k in ("oid", "hash", "priv"))
        code, sig = eng.bignSign2(P, oid, h, d, t)
        assert code == x["code"], x
        if code == 0:
            assert sig.hex() == x["sig"], x
            assert eng.bignVerify(P, oid, h, sig, eng.bignPubkeyCalc(P, d)[1]) == 0
    for x in ent["sign"]:
        rng = eng.rng_from_bytes(bytes.fromhex(x["rnd"]))
        code, sig = eng.bignSign(P, bytes.fromhex(x["oid"]), bytes.fromhex(x["hash"]), bytes.fromhex(x["priv"]), rng)
        assert code == x["code"], x
        if code == 0:
            assert (sig.hex(), rng.pos[0]) == (x["sig"], x["used"])
        else:
            assert rng.pos[0] == 0


def test_generic_sign_batch_and_verify_roundtrip():
    """a batch of a few hundred deterministic signatures on a non-standard set through bee2hip_bignSign2_batch, every one
    verified by bee2hip_bignVerify_batch on the same set, plus refused keys in the middle of the batch"""
    eng = engine()
    c = FIX["curves"][SFIX[0]["curve"]]
    P = mk(c)
    no = c["l"] // 4
    q = int.from_bytes(bytes.fromhex(c["q"]), "little")
    rnd = random.Random(99)
    n = 200
    privs = [rnd.randrange(1, q).to_bytes(no, "little") for _ in range(n)]
    privs[17] = bytes(no)
    privs[150] = q.to_bytes(no, "little")
    hs = [rnd.randbytes(no) for _ in range(n)]
    oid = bytes.fromhex(SFIX[0]["sign2"][0]["oid"])
    code, sigs, codes = eng.bignSign2_batch(P, oid, b"".join(hs), b"".join(privs), None)
    assert code == 0
    assert [i for i in range(n) if codes[i] != 0] == [17, 150] and codes[17] == codes[150] == 504
    good = [i for i in range(n) if codes[i] == 0]
    pcode, pubs, pcodes = eng.bignPubkeyCalc_batch(P, b"".join(privs[i] for i in good))
    assert pcode == 0 and all(x == 0 for x in pcodes)
    sg = no + no // 2
    vcode, vcodes = eng.bignVerify_batch(b"".join(hs[i] for i in good), b"".join(sigs[sg * i: sg * i + sg] for i in good), pubs,
                                         oid_der=oid, params=P)
    assert vcode == 0 and all(x == 0 for x in vcodes)


# ---- adversarial moduli, the exceptional branches of the ladder, launch geometry (tools/make_golden_generic_adv.py) ----
AFIX = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bign_generic_adv.json")))
CASE_EVENT = {"T == E": "add T == E", "T == -E": "add T == -E", "T == E later": "add T == E", "Y == 0 doubling": "dbl Y == 0",
              "R == O": "R == O"}


def _triples(cases):
    return tuple(b"".join(bytes.fromhex(x[f]) for x in cases) for f in ("hash", "sig", "pubkey"))


def test_adversarial_sets_verify_valid_and_damaged_signatures(orc):
    """every parameter set of bign_generic_adv.json (the smallest / largest prime, n0 = 1, low limb 3, an all-zero and an
    all-ones interior limb; q = 2^(2l) - 1, 2^(2l-1) + 1, n0(q) = 0xFFFFFFFF; a curve with a point of order 2; fresh
    isomorphic images): no-wrap valid signatures with full-size hashes (hashes beyond q among them) and their single-bit
    corruptions, one bee2hip_bignVerify_batch call per set, against orc_generic.verify"""
    eng = engine()
    seen = set()
    for si, s in enumerate(AFIX["sets"]):
        prm, P = mk(s), OG.Params.from_hex(s)
        cases = [x for x in AFIX["verify"] if x["set"] == si]
        assert len(cases) >= 5
        want = [OG.verify(P, bytes.fromhex(x["oid"]), bytes.fromhex(x["hash"]), bytes.fromhex(x["sig"]), bytes.fromhex(x["pubkey"]),
                          orc.belt_hash) for x in cases]
        assert want == [x["code"] for x in cases] and want.count(0) >= 2 and 510 in want
        code, got = eng.bignVerify_batch(*_triples(cases), oid_der=bytes.fromhex(cases[0]["oid"]), params=prm)
        assert code == 0 and got == want, (si, s["kind"], s["p_kind"], s["q_kind"], got, want)
        seen.add((s["l"], s["kind"], s["p_kind"], s["q_kind"]))
    assert len(seen) == 27


def test_exceptional_branches_of_the_verification_ladder(orc):
    """signatures crafted so that the simultaneous double-and-add of bign_generic_verify_kernel takes a branch random keys
    reach with probability 2^-l -- all but the last VALID, so a wrong branch turns an accept into a reject:
      T == E        Q = G, k = 3 2^l + t: u = k - (s0 + 2^l) has bit l as its top bit like v, so T = G when Q = G is added;
      T == -E       Q = -G, k = t small: u = t + s0 + 2^l, T = G when -G is added, the ladder goes on from O;
      T == E later  Q = 2 G, k = 5 2^l + t: where u = k - 2 (s0 + 2^l) has bit l + 1 as its top bit, T = G is doubled first and
                    meets Q as (X, Y, Z) with Z != 1 -- T == E in different representations (the tool keeps those that do);
      Y == 0        Q = (x0, 0) of order 2, u < 2^l, s0 of the parity that was guessed: T = Q at bit l, doubled next;
      R == O        Q = -G, H = 0 or q, s1 = s0 + 2^l: u = v, the sum is O and the verdict ERR_BAD_SIG.
    orc_generic.ladder_events replays the ladder on affine points and has to name the branch BEFORE the GPU is asked;
    the verdicts are orc_generic.verify's."""
    eng = engine()
    kinds = set()
    for si, s in enumerate(AFIX["sets"]):
        cases = [x for x in AFIX["crafted"] if x["set"] == si]
        if not cases:
            assert s["kind"] == "adv"
            continue
        prm, P = mk(s), OG.Params.from_hex(s)
        l = s["l"]
        want = []
        for x in cases:
            h, sg, k = (bytes.fromhex(x[f]) for f in ("hash", "sig", "pubkey"))
            ev = OG.ladder_events(P, h, sg, k)
            hit = [i for e, i in ev if e == CASE_EVENT[x["name"]]]
            assert hit, (si, x["name"], ev)
            if x["name"] in ("T == E", "T == -E", "T == E later"):
                assert l in hit
            assert (x["name"] == "T == E later") == (ev[0] == ("add T == E", l) and any(k[:l // 4]))          # Q = 2 G, not G
            if x["name"] == "Y == 0 doubling":
                assert l - 1 in hit
            want.append(OG.verify(P, bytes.fromhex(x["oid"]), h, sg, k, orc.belt_hash))
            assert want[-1] == x["code"] == (510 if x["name"] == "R == O" else 0), (si, x["name"])
            kinds.add((l, s["kind"], x["name"]))
        code, got = eng.bignVerify_batch(*_triples(cases), oid_der=bytes.fromhex(cases[0]["oid"]), params=prm)
        assert code == 0
        assert got == want, (si, s["kind"], [(x["name"], g) for x, g, w in zip(cases, got, want) if g != w])
        for x in cases[:2] + cases[-1:]:                    # the one-signature entry takes the same kernels
            assert eng.bignVerify(prm, *(bytes.fromhex(x[f]) for f in ("oid", "hash", "sig", "pubkey"))) == x["code"]
    for l in (128, 192, 256):
        assert {n for ll, k, n in kinds if ll == l and k == "tors"} == set(CASE_EVENT), l
        assert {n for ll, k, n in kinds if ll == l and k == "iso"} == set(CASE_EVENT) - {"Y == 0 doubling"}, l


def _scalars(l, q, rnd):
    """private / one-time keys: 1, 2, q - 1, powers of two, alternating limbs, refused ones (0, q, 2^(2l) - 1) in the middle"""
    alt = sum(0xFFFFFFFF << (64 * i) for i in range(l // 32))
    vals = [rnd.randrange(1, q), 1, 2, 0, q - 1, 1 << 31, 1 << 32, q, 1 << l, 1 << (2 * l - 2), (1 << (2 * l)) - 1, alt % q or 1, (alt << 32) % q or 1,
            rnd.randrange(1, q)]
    return vals


def test_adversarial_sets_signing_side(orc):
    """bee2hip_bignPubkeyCalc_batch and bee2hip_bignSignK_batch on every adversarial set but the ones with a point of order 2
    (k G there goes through formulas that are complete for odd order only), the special q's included: the arithmetic mod q of
    the signing tail runs over 2^(2l) - 1, 2^(2l-1) + 1 and a q with n0 = 0xFFFFFFFF.  Expected values: orc_generic.pubkey_calc /
    sign_k (pinned to the reference in tests/test_oracle_golden.py); refused items in mid-batch leave zeros."""
    eng = engine()
    for si, s in enumerate(AFIX["sets"]):
        if s["kind"] == "tors":
            continue
        prm, P = mk(s), OG.Params.from_hex(s)
        l = s["l"]
        no = l // 4
        q = OG.le(bytes.fromhex(s["q"]))
        rnd = random.Random(0x5100 + si)
        oid = bytes.fromhex([x for x in AFIX["verify"] if x["set"] == si][0]["oid"])
        enc = lambda v: v.to_bytes(no, "little")
        ds = _scalars(l, q, rnd)
        want = [OG.pubkey_calc(P, enc(d)) for d in ds]
        code, pubs, codes = eng.bignPubkeyCalc_batch(prm, b"".join(enc(d) for d in ds))
        assert code == 0 and codes == [c for c, _ in want], (si, codes)
        assert codes.count(504) == 3
        for i, (c, pk) in enumerate(want):
            assert pubs[2 * no * i: 2 * no * (i + 1)] == (pk if c == 0 else bytes(2 * no)), (si, s["p_kind"], s["q_kind"], hex(ds[i]))
        ks = _scalars(l, q, rnd)[::-1]
        ds2 = [d if 0 < d < q or i % 2 else 1 for i, d in enumerate(ds)]           # some refused d beside a refused k, most not
        hs = [enc(v) for v in (q, q + 1 if q + 1 < 1 << (2 * l) else q, (1 << (2 * l)) - 1, 0, q - 1)] + [rnd.randbytes(no) for _ in range(len(ds) - 5)]
        want = [OG.sign_k(P, oid, h, enc(d), enc(k), orc.belt_hash) for h, d, k in zip(hs, ds2, ks)]
        code, sigs, codes = eng.bignSignK_batch(prm, oid, b"".join(hs), b"".join(enc(d) for d in ds2), b"".join(enc(k) for k in ks))
        assert code == 0 and codes == [c for c, _ in want], (si, codes, [c for c, _ in want])
        assert 504 in codes and 304 in codes and codes.count(0) >= 8
        sg = no + no // 2
        for i, (c, sig) in enumerate(want):
            assert sigs[sg * i: sg * (i + 1)] == (sig if c == 0 else bytes(sg)), (si, s["p_kind"], s["q_kind"], i, hex(ds2[i]), hex(ks[i]))
        # records of the fixture (the reference's on the isomorphic sets)
        for x in [x for x in AFIX["sign_k"] if x["set"] == si]:
            code, sig, codes = eng.bignSignK_batch(prm, *(bytes.fromhex(x[f]) for f in ("oid", "hash", "priv", "k")))
            assert code == 0 and codes == [x["code"]] and (x["code"] or sig.hex() == x["sig"]), x
        for x in [x for x in AFIX["pubkey_calc"] if x["set"] == si]:
            code, pk = eng.bignPubkeyCalc(prm, bytes.fromhex(x["priv"]))
            assert code == x["code"] and (code or pk.hex() == x["pub"]), x


@pytest.mark.parametrize("l", (128, 192, 256))
def test_generic_batches_at_wavefront_boundaries(orc, l):
    """one lane per item, 64 lanes per block: n = 1, 63, 64, 65, 1000 through every generic batch entry, refused items
    (early-return lanes: a coordinate >= p, s1 >= q, d = 0, d >= q, k = q) next to working ones in every wavefront, every
    output compared item by item; refused items leave zeros.  The expected values of the distinct items come from
    orc_generic; the deterministic signatures of bignSign2 must be equal for equal inputs, verify under orc_generic.verify, be
    refused exactly where the key is out of range, and equal orc_sign2.sign2 (the Python restatement of their one-time key; q is
    the standard one here, so its loop makes one pass -- tests/test_gpu_bign_sign2_loop.py has the q's that make more)."""
    eng = engine()
    si, s = [(i, x) for i, x in enumerate(AFIX["sets"]) if x["l"] == l and x["kind"] == "iso"][0]
    prm, P = mk(s), OG.Params.from_hex(s)
    no = l // 4
    sg = no + no // 2
    q = OG.le(bytes.fromhex(s["q"]))
    rnd = random.Random(0x6E0 + l)
    enc = lambda v: v.to_bytes(no, "little")
    vc = [x for x in AFIX["verify"] if x["set"] == si]
    oid = bytes.fromhex(vc[0]["oid"])
    # verification pool: working, refused, working, ... (9 items: every 64 consecutive lanes hold them all, at shifting lanes)
    vpool = [tuple(bytes.fromhex(x[f]) for f in ("hash", "sig", "pubkey")) for x in vc]
    h, sig, k = vpool[0]
    vpool = [vpool[0], (h, sig, b"\xff" * no + k[no:]), vpool[1], (h, sig[:no // 2] + b"\xff" * no, k), vpool[2], vpool[3],
             (h, sig, k[:no] + b"\xff" * no), vpool[4], (h, sig[:no // 2] + enc(q), k)]
    vwant = [OG.verify(P, oid, *x, orc.belt_hash) for x in vpool]
    assert vwant.count(505) == 2 and 510 in vwant and vwant.count(0) == 2
    pvwant = [OG.pubkey_val(P, x[2]) for x in vpool]
    # signing pool: d, k, hash
    dpool = [rnd.randrange(1, q), 0, rnd.randrange(1, q), q, 1, rnd.randrange(1, q), (1 << (2 * l)) - 1]
    kpool = [rnd.randrange(1, q), 5, q, rnd.randrange(1, q), 0, q - 1, 7]
    hpool = [rnd.randbytes(no) for _ in range(5)] + [enc(q), enc((1 << (2 * l)) - 1)]
    pcwant = [OG.pubkey_calc(P, enc(d)) for d in dpool]
    skwant = [OG.sign_k(P, oid, hh, enc(d), enc(kk), orc.belt_hash) for hh, d, kk in zip(hpool, dpool, kpool)]
    assert [c for c, _ in skwant] == [0, 504, 304, 504, 304, 0, 504]
    s2ref = {}
    for n in (1, 63, 64, 65, 1000):
        iv = [i % len(vpool) for i in range(n)]
        code, got = eng.bignVerify_batch(*(b"".join(vpool[i][f] for i in iv) for f in range(3)), oid_der=oid, params=prm)
        assert code == 0 and got == [vwant[i] for i in iv], (n, [j for j, i in enumerate(iv) if got[j] != vwant[i]][:5])
        code, got = eng.bignPubkeyVal_batch(b"".join(vpool[i][2] for i in iv), prm)
        assert code == 0 and got == [pvwant[i] for i in iv], n
        ip = [(3 * i) % len(dpool) for i in range(n)]
        code, pubs, codes = eng.bignPubkeyCalc_batch(prm, b"".join(enc(dpool[i]) for i in ip))
        assert code == 0 and codes == [pcwant[i][0] for i in ip], n
        assert pubs == b"".join(pcwant[i][1] or bytes(2 * no) for i in ip), n
        code, sigs, codes = eng.bignSignK_batch(prm, oid, b"".join(hpool[i] for i in ip), b"".join(enc(dpool[i]) for i in ip),
                                                b"".join(enc(kpool[i]) for i in ip))
        assert code == 0 and codes == [skwant[i][0] for i in ip], n
        assert sigs == b"".join(skwant[i][1] or bytes(sg) for i in ip), n
        code, sigs, codes = eng.bignSign2_batch(prm, oid, b"".join(hpool[i] for i in ip), b"".join(enc(dpool[i]) for i in ip), None)
        assert code == 0 and codes == [0 if 0 < dpool[i] < q else 504 for i in ip], n
        for j, i in enumerate(ip):
            one = sigs[sg * j: sg * (j + 1)]
            if codes[j]:
                assert one == bytes(sg), (n, j)
            else:
                assert s2ref.setdefault(i, one) == one, (n, j)
    assert sorted(s2ref) == [i for i, d in enumerate(dpool) if 0 < d < q]
    for i, one in s2ref.items():
        assert OG.verify(P, oid, hpool[i], one, pcwant[i][1], orc.belt_hash) == 0, i
        assert S2.sign2(P, oid, hpool[i], enc(dpool[i]), None, orc.belt_hash, orc.wbl) == (0, one), i
