"""GPU: the one-time key of bignSign2 beyond its first pass (bign_sign_nonce_kernel, bign_sign_kernels.hip: k <- belt-wbl_theta(k)
until 0 < k < q).  On the standard curves a pass is rejected with probability below 2^-126, so everywhere else in the suite the
loop body runs once; here q = 2^(2l-1) + 1 and other non-standard q's reject up to one draw in two, lanes of one wavefront
finish at different passes, and the sticky done mask, the select that keeps a finished lane's k, the restart of the round
counter and the wavefront-wide exit all do work.

The batches come from tests/sign2plans.py (tests/test_sign2_model.py shows what pass counts each holds); the expected one-time
keys from tests/orc_sign2.py, pinned to the reference by tests/golden/bign_sign2_nonce.json.  EVERY item of every batch is
checked twice: the signature is byte-equal to bee2hip_bignSignK_batch's on the model's k (SignK is held to the Python signing
tail by test_gpu_bign_generic.py::test_adversarial_sets_signing_side), and the k recovered from the signature alone,
k = s1 + (s0 + 2^l) d + H mod q, is the model's -- which tells a wrong key from a wrong tail.  A handful per level goes through
the Python tail in full (orc_generic.sign_k), with nothing of the product in between: 8 per level -- 5 of the mixed batch of 65,
the late lane of one straggler batch, the early lane of one early-bird batch, one item on the "random odd" set.

The host path (host_bign_ct.hpp sign<N>) has the same loop but serves the standard curves only; see tests/test_sign2_model.py."""
import ctypes
import functools

import pytest

import orc_generic as OG
import orc_sign2 as S2
import sign2plans as PL
from gpulib import engine
from test_gpu_bign_generic import mk

pytestmark = pytest.mark.gpu
_sz = ctypes.c_size_t


@functools.lru_cache(None)
def _prm(si):
    return mk(PL.AFIX["sets"][si])


def _join(b):
    no = b.l // 4
    return (b"".join(it.h for it in b.items), b"".join(it.d for it in b.items),
            b"".join((1 if it.k is None else it.k).to_bytes(no, "little") for it in b.items))


def check_sigs(b, code, sigs, codes):
    """refused keys: 504 and zeros; every other item holds the model's k"""
    no, sg = b.l // 4, 3 * b.l // 8
    q = PL.q_of(b.si)
    assert code == 0 and len(sigs) == sg * len(b.items), (b.name, code)
    assert codes == [504 if it.k is None else 0 for it in b.items], (b.name, codes)
    for i, it in enumerate(b.items):
        one = sigs[sg * i: sg * (i + 1)]
        if it.k is None:
            assert one == bytes(sg), (b.name, i)
        else:
            assert S2.recover_k(b.l, q, one, it.d, it.h) == it.k, (b.name, i, "lane", i % 64, "passes", it.passes)


def run(eng, b, anchor=()):
    """bee2hip_bignSign2_batch on the batch, checked per item; anchor: items that also go through orc_generic.sign_k"""
    hs, ds, ks = _join(b)
    prm = _prm(b.si)
    code, sigs, codes = eng.bignSign2_batch(prm, b.oid, hs, ds, b.t)
    check_sigs(b, code, sigs, codes)
    kcode, ksigs, kcodes = eng.bignSignK_batch(prm, b.oid, hs, ds, ks)
    assert (kcode, kcodes) == (0, codes), b.name
    sg = 3 * b.l // 8
    assert ksigs == sigs, (b.name, [i for i in range(len(b.items)) if ksigs[sg * i: sg * (i + 1)] != sigs[sg * i: sg * (i + 1)]][:8])
    if anchor:
        import orclib
        P = OG.Params.from_hex(PL.AFIX["sets"][b.si])
        for i in anchor:
            it = b.items[i]
            want = OG.sign_k(P, b.oid, it.h, it.d, it.k.to_bytes(b.l // 4, "little"), orclib.load().belt_hash)
            assert want == (0, sigs[sg * i: sg * (i + 1)]), (b.name, i)
    return sigs


@pytest.mark.parametrize("l", PL.LEVELS)
@pytest.mark.parametrize("n", PL.MIXED_N)
def test_mixed_pass_counts_in_every_wavefront(l, n):
    """n = 1 (>= 4 passes), 63, 64, 65 (item 64 loops alone in its wavefront), 257, 1025: every full wavefront has a lane that
    is done after one pass next to one that needs four or more; hashes 0, q - 1, q and beyond, refused keys in wavefront 0.
    (n = 1 cannot tell whether a finished lane keeps its k: the loop ends with its only lane.)"""
    eng = engine()
    b = PL.mixed(l, n)
    anchor = ()
    if n == 65:          # 5 of the level's 8 anchors: the 1-pass lane, H = q, the >= 6-pass lane, the late lane, the last item
        anchor = (3, 5, 30, 40, 64)
        assert b.items[3].passes == 1 and b.items[30].passes >= 6 and b.items[40].passes >= 4
    sigs = run(eng, b, anchor)
    if n == 1:
        assert b.items[0].passes >= 4
    if n == 1025:        # the same items in another wavefront mix give the same signatures: nothing leaks between lanes
        sg = 3 * l // 8
        sub = PL.Batch("mixed, tail of 1025 on its own", b.si, l, b.oid, None, b.items[1000:])
        hs, ds, _ = _join(sub)
        code, again, codes = eng.bignSign2_batch(_prm(b.si), b.oid, hs, ds, None)
        assert code == 0 and again == sigs[sg * 1000:]


@pytest.mark.parametrize("l", PL.LEVELS)
@pytest.mark.parametrize("lane", PL.EDGE_LANES)
def test_one_late_lane_and_one_early_lane(l, lane):
    """one wavefront: `lane` alone needs >= 5 passes while 63 lanes hold their k from the first pass on; and the inverse, one
    lane whose k has to survive its neighbours' later passes.  A refused key sits in the looping wavefront each time."""
    eng = engine()
    run(eng, PL.straggler(l, lane), (lane,) if lane == 31 else ())
    run(eng, PL.early_bird(l, lane), (lane,) if lane == 32 else ())


@pytest.mark.parametrize("l", PL.LEVELS)
def test_every_rejecting_kind_of_q_and_the_control(l):
    """130 items on each "low limb 1" and "random odd" set, the "random odd" set with a point of order 2 included (k G there is
    outside what the kernels' formulas promise, so it takes part without the Python anchor: Sign2 against SignK and the
    recovered k hold whatever R is); on q = 2^(2l) - 1 nothing is ever rejected"""
    eng = engine()
    for kind in (PL.LOW1, PL.RANDOM_ODD, PL.ONES):
        sis = PL.set_indices(l, kind) + PL.set_indices(l, kind, "tors")
        assert len(sis) == {PL.LOW1: 2, PL.RANDOM_ODD: 2, PL.ONES: 2}[kind]
        for si in sis:
            b = PL.q_kind_batch(si)
            assert (max(it.passes for it in b.items) == 1) == (kind == PL.ONES)
            run(eng, b, (3,) if kind == PL.RANDOM_ODD and PL.AFIX["sets"][si]["kind"] == "adv" else ())


@pytest.mark.parametrize("l", PL.LEVELS)
@pytest.mark.parametrize("t_len", PL.T_DEVICE + PL.T_HOSTED,
                         ids=lambda v: f"t{v}_theta_in_the_nonce_kernel" if v in PL.T_DEVICE else f"t{v}_theta_from_the_ragged_hash_launch")
def test_both_theta_paths_with_a_loop_behind_them(l, t_len):
    """the shared additional input: none, 1, 31, 32, 33, 64 octets (theta hashed in the nonce kernel) and 65, 200 octets
    (theta from the ragged belt-hash launch), each with OIDs of every length mod 4, n = 65 on a rejecting set"""
    eng = engine()
    for oid_i in range(4):
        run(eng, PL.theta_batch(l, t_len, oid_i))


def _fixture_check(x, code, sig):
    s = PL.AFIX["sets"][x["set"]]
    assert code == x["code"] == 0, x
    d, h = bytes.fromhex(x["priv"]), bytes.fromhex(x["hash"])
    assert S2.recover_k(s["l"], PL.q_of(x["set"]), sig, d, h) == OG.le(bytes.fromhex(x["k"])), x
    if s["kind"] == "iso":               # elsewhere the reference's R is an artefact of its scalar recoding, its k is not
        assert sig.hex() == x["sig"], x


FIXTURE_SETS = sorted({x["set"] for x in PL.NFIX["records"]})


@pytest.mark.parametrize("si", FIXTURE_SETS, ids=lambda si: "set%d_l%d_%s" % (si, PL.AFIX["sets"][si]["l"], PL.AFIX["sets"][si]["kind"]))
@pytest.mark.parametrize("policy", (0, 1, 2))
def test_reference_records_through_the_drop_in_under_every_path_policy(policy, si):
    """EVERY record of bign_sign2_nonce.json through bignSign2(params, ...), one call each, a parameter set per case: a
    non-standard set has no host path, whatever the policy says (the host code's arithmetic mod q is made for the standard
    q's).  On the "iso" sets the whole signature is the reference's -- additional input of every length, both theta paths;
    elsewhere the one-time key is (the sets with a point of order 2 included)."""
    eng = engine()
    L = eng.lib
    recs = [x for x in PL.NFIX["records"] if x["set"] == si]
    assert len(recs) == 12
    was = L.bee2hip_path_policy(policy)
    try:
        for x in recs:
            before = L.bee2hip_path_count(0)
            code, sig = eng.bignSign2(_prm(si), bytes.fromhex(x["oid"]), bytes.fromhex(x["hash"]), bytes.fromhex(x["priv"]),
                                      None if x["t"] is None else bytes.fromhex(x["t"]))
            _fixture_check(x, code, sig)
            assert L.bee2hip_path_count(0) == before, ("host path taken", policy, si)
    finally:
        L.bee2hip_path_policy(was)


def test_multi_device_entry_on_a_rejecting_set():
    """bee2hip_bignSign2_batch_multi with ndev = 1: per item the model's k and, byte for byte, SignK on that k"""
    eng = engine()
    b = PL.mixed(192, 257)
    hs, ds, ks = _join(b)
    n, sg = len(b.items), 3 * b.l // 8
    sigs = ctypes.create_string_buffer(sg * n)
    codes = (ctypes.c_uint32 * n)()
    code = eng.lib.bee2hip_bignSign2_batch_multi(ctypes.byref(_prm(b.si)), b.oid, _sz(len(b.oid)), hs, ds, None, _sz(0), _sz(n), sigs, codes, 1)
    check_sigs(b, code, sigs.raw, list(codes))
    assert eng.bignSignK_batch(_prm(b.si), b.oid, hs, ds, ks) == (0, sigs.raw, list(codes))
