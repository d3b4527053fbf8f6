"""The one-time key of bignSign2 beyond its first pass, on the CPU: the Python model of STB 34.101.45 algorithm 6.3.3
(tests/orc_sign2.py on the C oracle's belt-hash and belt-wbl) against the records the reference made on rejecting q's
(tests/golden/bign_sign2_nonce.json, tools/make_golden_sign2_nonce.py) and against the C oracle's bignSign2 on the standard
curves; then the batches of tests/sign2plans.py, which tests/test_gpu_bign_sign2_loop.py sends through
bign_sign_nonce_kernel, are shown to hold the mixes of pass counts they are named after.

Not covered anywhere: the same loop in the host path (bee2_amd/csrc/host_bign_ct.hpp sign<N>).  That code serves the standard
curves only, its folds mod q rely on 2^(2l) - q being small, so it cannot be given another q without changing the product, and
on a standard q a second pass has probability below 2^-126: its later passes stay unreachable."""
import json
import os
import random

import pytest

import orc_generic as OG
import orc_sign2 as S2
import refgen
import sign2plans as PL
from bee2_amd.engine import LEVEL_OID

SETS = PL.AFIX["sets"]
RECORDS = PL.NFIX["records"]


def _rec(x):
    return tuple(None if x[f] is None else bytes.fromhex(x[f]) for f in ("oid", "priv", "t", "hash", "k", "sig"))


def test_fixture_covers_every_set_input_and_pass_count():
    per_set = {}
    for x in RECORDS:
        per_set.setdefault(x["set"], []).append(x)
    want = [i for i, s in enumerate(SETS) if s["kind"] != "iso"] + [i for i, s in enumerate(SETS) if s["kind"] == "iso"]
    assert sorted(per_set) == sorted(want) and len({SETS[i]["l"] for i in per_set if SETS[i]["kind"] == "iso"}) == 3
    for si, recs in per_set.items():
        q = PL.q_of(si)
        assert len(recs) >= 12 and all(x["code"] == 0 for x in recs)
        assert all(OG.le(bytes.fromhex(x["hash"])) < q and 0 < OG.le(bytes.fromhex(x["priv"])) < q for x in recs)     # H < q: see the tool
        assert {None if x["t"] is None else len(x["t"]) // 2 for x in recs} == {None, 1, 31, 32, 33, 64, 65, 200}
        assert {len(x["oid"]) // 2 % 4 for x in recs} == {0, 1, 2, 3}
    for l in PL.LEVELS:
        passes = [x["passes"] for x in RECORDS if SETS[x["set"]]["l"] == l and SETS[x["set"]]["q_kind"] == PL.HALF]
        assert {1, 2, 3, 4} <= set(passes) and max(passes) >= 6, (l, passes)


def test_model_matches_every_record_of_the_reference(orc):
    """k and the number of passes as the reference's replay, k as recovered from the reference's signature; on the sets whose q
    is the group order the whole signature"""
    for x in RECORDS:
        s = SETS[x["set"]]
        oid, d, t, h, k, sig = _rec(x)
        q = PL.q_of(x["set"])
        assert S2.nonce(oid, d, t, h, q, orc.belt_hash, orc.wbl) == (OG.le(k), x["passes"]), x
        assert S2.recover_k(s["l"], q, sig, d, h) == OG.le(k), x
        if s["kind"] == "iso":
            assert S2.sign2(OG.Params.from_hex(s), oid, h, d, t, orc.belt_hash, orc.wbl) == (0, sig), x


def test_model_refuses_keys_out_of_range_and_takes_no_t_as_empty_t(orc):
    si = PL.set_indices(128, PL.HALF)[0]
    P, q = OG.Params.from_hex(SETS[si]), PL.q_of(si)
    oid, h = PL.OIDS[1], bytes(range(32))
    for d in (0, q, (1 << 256) - 1):
        assert S2.sign2(P, oid, h, d.to_bytes(32, "little"), None, orc.belt_hash, orc.wbl) == (504, b"")
    d = (q - 2).to_bytes(32, "little")
    assert S2.nonce(oid, d, None, h, q, orc.belt_hash, orc.wbl) == S2.nonce(oid, d, b"", h, q, orc.belt_hash, orc.wbl)
    assert S2.nonce(oid, d, b"\0", h, q, orc.belt_hash, orc.wbl) != S2.nonce(oid, d, b"", h, q, orc.belt_hash, orc.wbl)


@pytest.mark.parametrize("l", PL.LEVELS)
def test_model_equals_the_c_oracle_on_the_standard_curves(orc, l):
    """the C oracle's bignSign2 (oracle/bign_oracle.c) against the model through recovery, and the whole signature once.
    The standard parameters are taken back from their isomorphic image in the fixture, (a, b, yG) -> (u^4 a, u^6 b, u^3 yG)
    with the same p and q: a = -3, u^2 = the square root of a' / a that is a square (p = 3 mod 4), b = b' / u^6,
    yG = b^((p+1)/4) as the standard has it -- and the sign of yG does not reach a signature, which holds x_R only."""
    no = l // 4
    std = [s for s in SETS if s["l"] == l and s["kind"] == "iso"][0]
    p, a_i, b_i, q = (OG.le(bytes.fromhex(std[f])) for f in ("p", "a", "b", "q"))
    u2 = pow(a_i * pow(p - 3, -1, p) % p, (p + 1) // 4, p)
    assert pow(u2, 2, p) * (p - 3) % p == a_i
    b = b_i * pow(u2, -3, p) % p
    P = OG.Params(l, *((v).to_bytes(no, "little") for v in (p, p - 3, b, q, pow(b, (p + 1) // 4, p))))
    rnd = random.Random(0x0C1E + l)
    oid = bytes(LEVEL_OID[l])
    whole = 0
    for t in (None, b"\x05", rnd.randbytes(100)):
        for _ in range(2):
            d, h = rnd.randrange(1, q).to_bytes(no, "little"), rnd.randbytes(no)
            code, sig = orc.sign2(l, oid, h, d, t)
            k, passes = S2.nonce(oid, d, t, h, q, orc.belt_hash, orc.wbl)
            assert code == 0 and passes == 1 and S2.recover_k(l, q, sig, d, h) == k
            if t == b"\x05" and not whole:
                assert OG.pubkey_calc(P, d) == orc.pubkey_calc(l, d)            # the parameters ARE the standard ones
                assert S2.sign2(P, oid, h, d, t, orc.belt_hash, orc.wbl) == (0, sig)
                whole += 1
    assert whole == 1


@pytest.mark.ref
@pytest.mark.skipif(not refgen.have_ref(), reason="oracle/_ref not built")
def test_fixture_regenerates_byte_identically(tmp_path):
    import make_golden_sign2_nonce as mg
    out, _ = mg.build()
    path = tmp_path / "again.json"
    json.dump(out, open(path, "w"), indent=0)
    assert open(path, "rb").read() == open(os.path.join(PL.HERE, "golden", "bign_sign2_nonce.json"), "rb").read()


# ---- what the GPU batches hold, from the model alone
@pytest.mark.parametrize("l", PL.LEVELS)
def test_mixed_batches_hold_early_and_late_lanes_in_every_full_wavefront(l):
    deepest = 0
    for n in PL.MIXED_N:
        b = PL.mixed(l, n)
        q = PL.q_of(b.si)
        assert len(b.items) == n and SETS[b.si]["q_kind"] == PL.HALF
        for w in PL.wavefronts(b):
            assert 1 in w and max(w) >= 4, (n, w)
        deepest = max(deepest, max(it.passes for it in b.items))
        if n >= 63:
            hs = {OG.le(it.h) for it in b.items}
            assert {q, 0, q - 1} <= hs and any(v > q for v in hs)
            assert [OG.le(it.d) for it in b.items if it.k is None] == list(PL.refused_keys(b.si))
            assert max(it.passes for it in b.items) >= 6
    assert len(PL.wavefronts(PL.mixed(l, 1025))) == 16
    assert PL.mixed(l, 1).items[0].passes >= 4
    last = PL.mixed(l, 65).items[64]
    assert last.passes >= 5 and last.k is not None            # one active lane loops alone in the last wavefront
    assert deepest >= 6


@pytest.mark.parametrize("l", PL.LEVELS)
def test_straggler_and_early_bird_batches_have_one_odd_lane(l):
    for lane in PL.EDGE_LANES:
        b = PL.straggler(l, lane)
        p = [it.passes for it in b.items]
        assert len(p) == 64 and p[lane] >= 5 and all(v == 1 for i, v in enumerate(p) if i != lane), (lane, p)
        b2 = PL.early_bird(l, lane)
        p = [it.passes for it in b2.items]
        assert len(p) == 64 and p[lane] == 1 and all(v >= 3 for i, v in enumerate(p) if i != lane), (lane, p)
        for x in (b, b2):                                       # a refused key inside the looping wavefront, not the odd lane
            bad = [i for i, it in enumerate(x.items) if it.k is None]
            assert bad == [(lane + 2) % 64] and x.items[lane].k is not None
    assert {OG.le(PL.straggler(l, lane).items[(lane + 2) % 64].d) for lane in PL.EDGE_LANES} == set(PL.refused_keys(PL.straggler(l, 0).si))


@pytest.mark.parametrize("l", PL.LEVELS)
def test_other_q_kinds_reject_and_the_all_ones_q_never_does(l):
    for kind in (PL.LOW1, PL.RANDOM_ODD):
        sis = PL.set_indices(l, kind) + PL.set_indices(l, kind, "tors")
        assert len(sis) == 2 and (kind == PL.LOW1 or [PL.AFIX["sets"][i]["kind"] for i in sis] == ["adv", "tors"])
        for si in sis:
            b = PL.q_kind_batch(si)
            p = [it.passes for it in b.items]
            assert len(p) == 130 and [i for i, it in enumerate(b.items) if it.k is None] == [64, 65, 66]
            assert all(1 in w and max(w) >= 3 for w in PL.wavefronts(b)), (si, sorted(p))
    for si in PL.set_indices(l, PL.ONES):
        assert {it.passes for it in PL.q_kind_batch(si).items} == {1}


@pytest.mark.parametrize("l", PL.LEVELS)
def test_theta_batches_cross_every_t_length_with_every_oid_length(l):
    for t_len in PL.T_DEVICE + PL.T_HOSTED:
        for oid_i in range(4):
            b = PL.theta_batch(l, t_len, oid_i)
            assert len(b.oid) % 4 == oid_i and len(b.t or b"") == t_len and len(b.items) == 65
            assert b.items[64].passes >= 3 and b.items[7].k is None and SETS[b.si]["q_kind"] == PL.LOW1
            assert max(it.passes for it in b.items[:64]) >= 2 and 1 in [it.passes for it in b.items[:64]]
