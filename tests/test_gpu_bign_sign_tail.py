"""-m gpu: the tail of signing, s1 = (k - (s0 + 2^l) d - H) mod q, of bign_sign_tail_kernel<8|12|16> (bee2_amd/csrc/bign_sign_kernels.hip:
mod_q_ct, then sub_mod_q_ct twice) in the branches no random draw reaches, bit for bit against tests/golden/bign_sign_tail.json
-- the reference's own octets for private keys that were SOLVED so that (s0 + 2^l) d mod q is 1, cq - 1, cq, q - 1, ..., for every
event of the fold the bound leaves possible, for k - r and u - H equal to 0 and q - 1, and for H >= q with and without a residue
coming out (tools/make_golden_sign_tail.py; tests/signtail.py restates the tail; tests/test_sign_tail_fixture.py proves on the
CPU that the file is what it says and that its coverage of the fold's events is complete).

Every entry that takes the one-time key from the caller is driven: bee2hip_bignSignK_batch (host pointers),
bee2hip_bignSignKL_batch_dev, bignSign through a replaying generator under both path policies; bee2hip_bignVerify_batch then
judges what the kernel wrote.  bign_generic_sign_tail_kernel, which reduces H first, gets the kinds with H < q on the isomorphic
images of the standard curves, with orc_generic.sign_k as its pin."""
import ctypes
import functools
import json
import os
import random

import pytest
import torch

import orc_generic as OG
import orclib
import signtail as T
from bee2_amd import engine as E
from gpulib import dev, engine, host

pytestmark = pytest.mark.gpu

SIZES = (64 + 3, 257)                      # one wavefront and a bit; a block of 256 and one lane
FILL, CFILL = 0xA5, 0x5A5A5A5A


def _params(eng, l):
    return eng.bignParamsStd(E.CURVE_NAME[l])


def _oids(l):
    """the two OIDs of the level's records, the level's own first"""
    own = bytes(E.LEVEL_OID[l])
    other = sorted({c["oid"] for c in T.load().of(l)} - {own})
    assert len(other) == 1 and len(other[0]) % 4 != len(own) % 4
    return own, other[0]


@functools.lru_cache(maxsize=None)
def _batch(l, oid, n):
    """-> list of (d, k, H, code, sig, what): all records of (l, oid) in ONE batch of n items.  Steered records in lane 0, in lanes 63
    and 64 and in the last lane; the others from lane 2 on with a refused item (d = 0, d = q, k = 0, k = q in turn) before each;
    seeded ordinary items, expected from the oracle, everywhere else.  Built once per (l, oid, n) and shared by the tests."""
    orc = orclib.load()
    no, sg = l // 4, 3 * l // 8
    q = T.curve_q(l)
    recs = [c for c in T.load().of(l) if c["oid"] == oid]
    assert 8 <= len(recs) and 2 * len(recs) < 63 < n
    rnd = random.Random(0x7A110000 + 1000 * l + n + len(oid))
    enc = lambda v: v.to_bytes(no, "little")
    slots = [None] * n
    item = lambda c: (c["priv"], c["k"], c["hash"], 0, c["sig"], c["kind"] + " " + c["name"])
    for pos, c in zip((0, 63, 64, n - 1), recs):
        slots[pos] = item(c)
    bad = [(0, None, 504, "refused d=0"), (q, None, 504, "refused d=q"), (None, 0, 304, "refused k=0"), (None, q, 304, "refused k=q")]
    for j, c in enumerate(recs[4:]):
        d, k, code, what = bad[j % 4]
        slots[1 + 2 * j] = (enc(rnd.randrange(1, q) if d is None else d), enc(rnd.randrange(1, q) if k is None else k), rnd.randbytes(no),
                            code, bytes(sg), what)
        slots[2 + 2 * j] = item(c)
    assert len(recs) - 4 >= 4
    for i in range(n):
        if slots[i] is None:
            d, k, h = enc(rnd.randrange(1, q)), enc(rnd.randrange(1, q)), rnd.randbytes(no)
            code, sig, used = orc.sign_rnd(l, oid, h, d, k)
            assert (code, used) == (0, 1)
            slots[i] = (d, k, h, 0, sig, "ordinary")
    assert sum(s[5].split()[0] in T.KINDS for s in slots) == len(recs)
    return slots


def _columns(slots):
    return (b"".join(s[f] for s in slots) for f in (0, 1, 2))


def _check(l, slots, codes, sigs, what):
    sg = 3 * l // 8
    assert len(codes) == len(slots) and len(sigs) == sg * len(slots)
    bad = [(i, s[5], codes[i], s[3]) for i, s in enumerate(slots) if codes[i] != s[3]]
    assert not bad, (what, bad[:8])
    bad = [(i, s[5]) for i, s in enumerate(slots) if sigs[sg * i: sg * (i + 1)] != s[4]]     # zeros where the item was refused
    assert not bad, (what, len(bad), bad[:12])


@pytest.mark.parametrize("l", T.LEVELS)
def test_signK_batch_host_pointers(l):
    """bee2hip_bignSignK_batch: codes, every signature's octets -- the "wrap" records' too, whose s1 is no residue --, zeros for
    the refused items, the ordinary items as the oracle"""
    eng = engine()
    P = _params(eng, l)
    for oid in _oids(l):
        for n in SIZES:
            slots = _batch(l, oid, n)
            ds, ks, hs = _columns(slots)
            code, sigs, codes = eng.bignSignK_batch(P, oid, hs, ds, ks)
            assert code == 0, (l, len(oid), n, code)
            _check(l, slots, codes, sigs, (l, len(oid), n))


@pytest.mark.parametrize("l", T.LEVELS)
def test_signKL_batch_dev_with_a_guard_slot_behind_the_outputs(l):
    """bee2hip_bignSignKL_batch_dev on the same batches: outputs pattern-filled, one more slot behind the signatures and behind
    the codes that must keep the pattern; the inputs stay as they were (the kernel wipes its own copy of the one-time keys)"""
    eng = engine()
    sg = 3 * l // 8
    for oid in _oids(l):
        for n in SIZES:
            slots = _batch(l, oid, n)
            ds, ks, hs = _columns(slots)
            td, tk, th = dev(ds), dev(ks), dev(hs)
            sigs = torch.full((sg * (n + 1),), FILL, dtype=torch.uint8, device="cuda")
            codes = torch.full((n + 1,), CFILL, dtype=torch.int32, device="cuda")
            eng.bignSignKL_batch_dev(l, oid, th, td, tk, sigs[: sg * n], codes[:n])
            torch.cuda.synchronize()
            got, gc = host(sigs), [int(c) & 0xFFFFFFFF for c in codes.cpu().numpy()]
            assert got[sg * n:] == bytes([FILL]) * sg and gc[n] == CFILL, "the guard slot behind the outputs was written"
            _check(l, slots, gc[:n], got[: sg * n], (l, len(oid), n))
            assert (host(td), host(tk), host(th)) == (ds, ks, hs)


@pytest.mark.parametrize("l", T.LEVELS)
def test_bignSign_drop_in_under_both_path_policies(l):
    """bignSign with a generator that replays the record's k, one record per call.  Policy 0: the single signature is made on
    the calling core (host_bign_ct.hpp) and bee2hip_path_count(0) says so, once per call.  Policy 1: the host path is not taken
    and nothing finishes on the host after a failure, so the call went where bignSign sends it then: bee2hip_bignSignK_batch
    with n = 1, the tail kernel with one lane.  Both give the reference's octets."""
    eng = engine()
    L = eng.lib
    P = _params(eng, l)
    recs = T.load().of(l)
    was = L.bee2hip_path_policy(-1)
    try:
        for policy in (0, 1):
            L.bee2hip_path_policy(policy)
            before = [L.bee2hip_path_count(i) for i in range(3)]
            for c in recs:
                rng = eng.rng_from_bytes(c["k"])
                code, sig = eng.bignSign(P, c["oid"], c["hash"], c["priv"], rng)
                assert (code, rng.pos[0]) == (0, l // 4) and sig == c["sig"], (policy, c["kind"], c["name"])
            after = [L.bee2hip_path_count(i) for i in range(3)]
            assert after[0] - before[0] == (len(recs) if policy == 0 else 0) and after[2] == before[2], (policy, before, after)
    finally:
        L.bee2hip_path_policy(was)
    assert L.bee2hip_path_policy(-1) == was


@pytest.mark.parametrize("l", T.LEVELS)
def test_verify_batch_judges_what_the_kernel_signed(l):
    """the records alone through bee2hip_bignSignK_batch, then bee2hip_bignVerify_batch on THOSE octets under the fixture's public
    keys: the reference's verdicts -- 0 everywhere, ERR_BAD_SIG on the "wrap" records, whose s1 is not below q"""
    eng = engine()
    P = _params(eng, l)
    sg = 3 * l // 8
    for oid in _oids(l):
        recs = [c for c in T.load().of(l) if c["oid"] == oid]
        hs = b"".join(c["hash"] for c in recs)
        code, sigs, codes = eng.bignSignK_batch(P, oid, hs, b"".join(c["priv"] for c in recs), b"".join(c["k"] for c in recs))
        assert code == 0 and codes == [0] * len(recs)
        assert [sigs[sg * i: sg * (i + 1)] for i in range(len(recs))] == [c["sig"] for c in recs]
        code, vcodes = eng.bignVerify_batch(hs, sigs, b"".join(c["pub"] for c in recs), oid_der=oid, params=P)
        assert code == 0 and vcodes == [c["verify"] for c in recs], [(c["kind"], c["name"], v) for c, v in zip(recs, vcodes) if v != c["verify"]]
        assert {c["verify"] for c in recs} == {0, T.ERR_BAD_SIG}
        assert all((c["verify"] != 0) == (c["kind"] == "wrap") for c in recs)


AFIX = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bign_generic_adv.json")))


def _mk(s):
    prm = E.bign_params()
    prm.l = s["l"]
    for f in ("p", "a", "b", "q", "yG"):
        raw = bytes.fromhex(s[f])
        ctypes.memmove(getattr(prm, f), raw + bytes(64 - len(raw)), 64)
    return prm


@pytest.mark.parametrize("l", T.LEVELS)
def test_generic_tail_on_the_isomorphic_set(orc, l):
    """bign_generic_sign_tail_kernel (Montgomery arithmetic mod q, H reduced first) on the "iso" parameter set of the level -- the
    standard q on another model of the curve, so s0 differs and the keys are solved here: u = 0 and q - 1, k = 1 and q - 1,
    s1 = 0, 1 and q - 1, H = 0 and q - 1.  Expected octets: orc_generic.sign_k; the integer model says each is the corner it
    is named after.  One batch through bee2hip_bignSignK_batch, a refused item in the middle."""
    eng = engine()
    si, s = [(i, x) for i, x in enumerate(AFIX["sets"]) if x["l"] == l and x["kind"] == "iso"][0]
    prm, P = _mk(s), OG.Params.from_hex(s)
    no, sg = l // 4, 3 * l // 8
    q = OG.le(bytes.fromhex(s["q"]))
    assert q == T.curve_q(l)
    oid = bytes.fromhex([x for x in AFIX["verify"] if x["set"] == si][0]["oid"])
    enc = lambda v: v.to_bytes(no, "little")
    rnd = random.Random(0x150 + l)
    items, corners = [], {}
    for kind, plan in (("sub1", T.plan_sub1), ("sub2", T.plan_sub2)):
        for name, k, H, r in plan(l, q, rnd):
            code, first = OG.sign_k(P, oid, enc(H), enc(1), enc(k), orc.belt_hash)
            assert code == 0
            s0 = T.le(first[:l // 8])
            d = r * pow(s0 + (1 << l), -1, q) % q
            code, want = OG.sign_k(P, oid, enc(H), enc(d), enc(k), orc.belt_hash)
            t = T.tail(l, q, s0, d, k, H)
            assert code == 0 and want[:l // 8] == first[:l // 8] and t["r"] == r and T.le(want[l // 8:]) == t["s1"] < q and H < q
            corners[name] = t
            items.append((enc(d), enc(k), enc(H), 0, want, kind + " " + name))
    assert (corners["u=0"]["u"], corners["u=q-1"]["u"], corners["s1=0"]["s1"], corners["s1=q-1"]["s1"]) == (0, q - 1, 0, q - 1)
    assert corners["u=0"]["r"] == T.le(items[0][1]) and corners["s1=0"]["u"] == T.le(items[5][2])          # k == r; u == H
    items.insert(5, (enc(q), enc(1), bytes(no), 504, bytes(sg), "refused d=q"))
    ds, ks, hs = _columns(items)
    code, sigs, codes = eng.bignSignK_batch(prm, oid, hs, ds, ks)
    assert code == 0
    _check(l, items, codes, sigs, ("iso", l))
