"""-m gpu: every host-pointer entry point through BOTH kinds of staging (bee2_amd/csrc/staging.hpp Stage / Scratch): the pinned,
device-mapped buffer that serves requests up to 64 KiB (2 KiB for the serial chains), and device memory with hipMemcpy, which the
pinned limit of the experiments build (bee2hip_internal_tune(3, 0)) forces for every size.  The shapes are the smallest at which
a part's offset, a copy skipped at length zero or a partial tail can go wrong: 0 / 1 / 15 / 16 / 17 / 31 / 32 / 33 / 48 octets,
both sides of the two limits, and host batches of 1 and 3 items at l = 192, where three signatures are 216 octets and the part
staged behind them really is rounded up.  The GPU path is forced (bee2hip_path_policy(1)); every octet is compared with the
oracle (bash-prg: with the model of tests/orc_bashprg.py, which tests/golden/bash_prg.json pins).

Path counts: the drop-in groups must raise bee2hip_path_count(1); the batch entries never go through the drop-in helper, so
for them the count may stand still.  No group may raise the host count (0) or the fallback count (2)."""
import ctypes
import random
import struct

import pytest

import orc_bashprg as M
from bee2_amd import engine as E
from gpulib import exp_engine

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 15, 16, 17, 31, 32, 33, 48)
_sz = ctypes.c_size_t


@pytest.fixture(params=["pinned", "device"])
def eng(request):
    """the experiments library on the forced GPU path, staging by the default limit or always in device memory"""
    e = exp_engine()
    L = e.lib
    L.bee2hip_path_policy(1)
    L.bee2hip_internal_tune(3, 65536 if request.param == "pinned" else 0)
    before = [L.bee2hip_path_count(i) for i in range(3)]
    try:
        yield e
        after = [L.bee2hip_path_count(i) for i in range(3)]
        assert after[0] == before[0], "a call took the host path under the forced GPU policy"
        assert after[2] == before[2], "a GPU path failed and was finished on the host"
    finally:
        L.bee2hip_internal_tune(3, 65536)
        L.bee2hip_path_policy(0)


def _gpu_calls(e):
    return e.lib.bee2hip_path_count(1)


def _split(n):
    """one split inside a block (of 16, 32 and 128 octets alike) wherever the length allows one"""
    a = n // 2 + (1 if n // 2 % 16 == 0 and n > 2 else 0)
    return [a, n - a]


@pytest.fixture(scope="module")
def kv(orc):
    H = orc.beltH()
    return H[128:160], H[192:208]


# ================================================================================================ streaming and one-shot drop-ins
def test_bash_hash_and_bashF(eng, orc):
    g0 = _gpu_calls(eng)
    # sponge_gpu stages state || data as a chain: 1632 octets of data fill 2048 exactly, 1633 go to device memory
    for n in SIZES + (127, 128, 129, 1632, 1633, 2048, 2049):
        msg = orc.fill(n, 0x5A00 + n)
        want = orc.bashHash(128, msg)[1]
        assert eng.bashHash(128, msg) == (0, want), n
        assert eng.bashHash_steps(128, msg, _split(n)) == (want, True), n
    st = orc.fill(192, 0x5AF)
    assert eng.bashF(st) == orc.bashF(st)
    assert eng.bashF_batch(st * 3) == orc.bashF(st) * 3
    assert _gpu_calls(eng) > g0


def test_belt_ctr_mac_hash(eng, orc, kv):
    key, iv = kv
    g0 = _gpu_calls(eng)
    # CTR stages whole blocks and one more for the gamma: 65520 octets fill the pinned buffer exactly
    for n in SIZES + (65520, 65536, 65537):
        msg = orc.fill(n, 0xC700 + n)
        want = orc.ctr(msg, key, iv)
        assert eng.beltCTR(msg, key, iv) == (0, want), n
        if n < 100:
            assert eng.beltCTR_steps(msg, key, iv, _split(n))[0] == want, n
    for n in SIZES:
        msg = orc.fill(n, 0x3AC0 + n)
        want = orc.mac(msg, key)
        assert eng.beltMAC(msg, key) == (0, want), n
        assert eng.beltMAC_steps(msg, key, _split(n)) == (want, True), n
    # belt-hash stages data || state + 64 as a chain: 1984 octets of data make 2048, 2016 go to device memory
    for n in SIZES + (1984, 2016, 2048, 2049):
        msg = orc.fill(n, 0x4A50 + n)
        assert eng.beltHash(msg) == (0, orc.belt_hash(msg)), n
        a, b = _split(n)
        assert eng.beltHash_steps(msg, [a, b]) == [orc.belt_hash(msg[:a]), orc.belt_hash(msg)], n
    assert _gpu_calls(eng) > g0


def test_belt_block_modes(eng, orc, kv):
    key, iv = kv
    g0 = _gpu_calls(eng)
    for n in (16, 17, 31, 32, 33, 48):
        msg = orc.fill(n, 0xEC0 + n)
        for decr in (False, True):
            d = "Decr" if decr else "Encr"
            assert eng.belt_mode("beltECB" + d, msg, key) == orc.ecb(msg, key, decr), (n, d)
            assert eng.belt_mode("beltCBC" + d, msg, key, iv) == orc.cbc(msg, key, iv, decr), (n, d)
            if n % 16 == 0:
                assert eng.belt_mode("beltBDE" + d, msg, key, iv) == orc.bde(msg, key, iv, decr), (n, d)
            if n % 16 == 0 and n >= 32:
                assert eng.belt_mode("beltSDE" + d, msg, key, iv) == orc.sde(msg, key, iv, decr), (n, d)
    blk = orc.fill(16, 0xB10C)
    assert eng.beltBlockEncr(blk, key) == orc.block_encr(blk, key)
    assert eng.beltBlockDecr(blk, key) == orc.block_decr(blk, key)
    assert _gpu_calls(eng) > g0


@pytest.mark.parametrize("mode", ["DWP", "CHE"])
def test_belt_dwp_che_wrap_unwrap(eng, orc, kv, mode):
    key, iv = kv
    g0 = _gpu_calls(eng)
    for i, n in enumerate(SIZES):
        crit, open_ = orc.fill(n, 0xD00 + n), orc.fill(SIZES[(i + 4) % len(SIZES)], 0xD80 + n)
        code, ct, mac = orc.dwp_wrap(crit, open_, key, iv, mode)
        assert code == 0 and eng.dwp_wrap(crit, open_, key, iv, mode) == (0, ct, mac), n
        assert eng.dwp_unwrap(ct, open_, mac, key, iv, mode) == (0, crit), n
        bad = bytes([mac[0] ^ 1]) + mac[1:]
        assert eng.dwp_unwrap(ct, open_, bad, key, iv, mode)[0] == E.ERR_BAD_MAC, n
    assert _gpu_calls(eng) > g0


# ================================================================================================ host batches
L192 = 192


@pytest.fixture(scope="module")
def signed(orc):
    """four signatures at l = 192 by two signers (the oracle's), the third one damaged: (privs, pubs, hashes, sigs, codes, who)"""
    no, oid = L192 // 4, E.LEVEL_OID[L192]
    privs = [orc.fill(no - 1, 0x9100 + i) + b"\x3f" for i in range(2)]
    pubs = [orc.pubkey_calc(L192, d)[1] for d in privs]
    hashes = [orc.fill(no, 0x9200 + i) for i in range(4)]
    who = [0, 1, 0, 0]
    sigs = [orc.sign2(L192, oid, hashes[i], privs[who[i]])[1] for i in range(4)]
    sigs[2] = sigs[2][:5] + bytes([sigs[2][5] ^ 4]) + sigs[2][6:]
    codes = [orc.verify_l(L192, oid, hashes[i], sigs[i], pubs[who[i]]) for i in range(4)]
    assert codes[0] == codes[1] == codes[3] == 0 and codes[2] != 0
    return privs, pubs, hashes, sigs, codes, who


@pytest.mark.parametrize("n", [1, 3])
def test_bign_verify_and_pubkey_batches(eng, orc, signed, n):
    privs, pubs, hashes, sigs, codes, who = signed
    P, oid = eng.bignParamsStd(E.CURVE_NAME[L192]), E.LEVEL_OID[L192]
    pick = [2] if n == 1 else [0, 1, 2]                      # n = 1: the damaged one, n = 3: 216 octets of signatures
    hs, ss = b"".join(hashes[i] for i in pick), b"".join(sigs[i] for i in pick)
    want = [codes[i] for i in pick]
    assert eng.bignVerify_batch(hs, ss, b"".join(pubs[who[i]] for i in pick), oid, P) == (0, want)
    assert eng.bignVerify_keyed_batch(hs, ss, b"".join(pubs), [who[i] for i in pick], oid, P) == (0, want)
    mine = [2] if n == 1 else [0, 2, 3]                      # signer 0's
    assert eng.bignVerify_onekey_batch(b"".join(hashes[i] for i in mine), b"".join(sigs[i] for i in mine), pubs[0], oid, P) == \
        (0, [codes[i] for i in mine])
    keys = [pubs[0], pubs[1][:7] + bytes([pubs[1][7] ^ 1]) + pubs[1][8:], pubs[1]][:n]
    assert eng.bignPubkeyVal_batch(b"".join(keys), P) == (0, orc.pubkey_val_batch(L192, b"".join(keys)))
    ds = [privs[0], bytes(L192 // 4), privs[1]][:n]          # (the zero key is refused: its slot of the output stays as it was)
    code, out, cs = eng.bignPubkeyCalc_batch(P, b"".join(ds))
    ref = [orc.pubkey_calc(L192, d) for d in ds]
    assert code == 0 and cs == [r[0] for r in ref]
    assert out == b"".join(r[1] if r[0] == 0 else bytes(L192 // 2) for r in ref)


@pytest.mark.parametrize("n", [1, 3])
def test_bign_sign_batches(eng, orc, signed, n):
    privs, _, hashes, _, _, who = signed
    P, oid, no = eng.bignParamsStd(E.CURVE_NAME[L192]), E.LEVEL_OID[L192], L192 // 4
    hs, ds = b"".join(hashes[:n]), b"".join(privs[who[i]] for i in range(n))
    for t_len in (0, 64, 65):                                 # 65: beyond the nonce kernel's own 64, theta through slot 2
        t = orc.fill(t_len, 0x7E7A) if t_len else None
        want = [orc.sign2(L192, oid, hashes[i], privs[who[i]], t) for i in range(n)]
        assert eng.bignSign2_batch(P, oid, hs, ds, t) == (0, b"".join(w[1] for w in want), [w[0] for w in want]), t_len
    ks = [orc.fill(no - 1, 0x6B00 + i) + b"\x3f" for i in range(n)]
    want = [orc.sign_rnd(L192, oid, hashes[i], privs[who[i]], ks[i]) for i in range(n)]
    assert all(w[0] == 0 for w in want)
    assert eng.bignSignK_batch(P, oid, hs, ds, b"".join(ks)) == (0, b"".join(w[1] for w in want), [0] * n)


@pytest.mark.parametrize("n", [1, 3])
def test_bash_hash_belt_mac_batch(eng, orc, kv, n):
    key = kv[0]
    for msg_len in (0, 1, 17):
        msgs = [orc.fill(msg_len, 0x4D00 + 8 * msg_len + i) for i in range(n)]
        dig, tag = eng.bashHash_beltMAC_batch(b"".join(msgs), msg_len, 256, key, n=n)
        assert dig == b"".join(orc.bashHash(256, m)[1] for m in msgs), msg_len
        assert tag == b"".join(orc.mac(m, key) for m in msgs), msg_len


def test_bash_prg_ragged_records_that_start_at_offset_5(eng):
    """three records of 0, 1 and 17 octets whose first offset is 5: the staged text keeps its alignment mod 16"""
    L = eng.lib
    l, d, lens = 192, 1, (0, 1, 17)
    rnd = random.Random(0x5747)
    offs = [5]
    for k in lens:
        offs.append(offs[-1] + k)
    blob = rnd.randbytes(offs[-1] + 3)
    texts = [blob[offs[i]:offs[i + 1]] for i in range(3)]
    qoffs = struct.pack("<4Q", *offs)
    ann = rnd.randbytes(8)
    out = ctypes.create_string_buffer(3 * 24)
    assert L.bee2hip_bashPrgHash_ragged(_sz(l), _sz(d), ann, _sz(8), blob, qoffs, _sz(3), out, _sz(24)) == 0
    assert out.raw == b"".join(M.prg_hash(l, d, ann, t, 24) for t in texts)
    key, anns, hdrs = rnd.randbytes(24), [rnd.randbytes(4) for _ in range(3)], [rnd.randbytes(k) for k in (17, 0, 1)]
    hblob, hoffs = b"\x00" * 5 + b"".join(hdrs), struct.pack("<4Q", 5, 22, 22, 23)
    want = [M.ae_wrap(l, d, key, anns[i], hdrs[i], texts[i], 16) for i in range(3)]
    guard = rnd.randbytes(len(blob))
    dst = ctypes.create_string_buffer(guard, len(blob))
    tags = ctypes.create_string_buffer(3 * 16)
    assert L.bee2hip_bashPrgAE_wrap_ragged(_sz(l), _sz(d), key, _sz(24), b"".join(anns), _sz(4), hblob, hoffs, blob, qoffs, _sz(3),
                                           dst, tags, _sz(16)) == 0
    ct = b"".join(w[0] for w in want)
    assert dst.raw == guard[:5] + ct + guard[5 + len(ct):]           # the text at its offset, nothing around it touched
    assert tags.raw == b"".join(w[1] for w in want)
    bad = bytearray(tags.raw)
    bad[16] ^= 1                                                      # record 1 is refused
    src = bytes(5) + ct + bytes(3)
    pt = ctypes.create_string_buffer(guard, len(blob))
    codes = (ctypes.c_uint32 * 3)()
    assert L.bee2hip_bashPrgAE_unwrap_ragged(_sz(l), _sz(d), key, _sz(24), b"".join(anns), _sz(4), hblob, hoffs, src, qoffs, _sz(3),
                                             bytes(bad), _sz(16), pt, codes) == 0
    assert list(codes) == [0, E.ERR_BAD_MAC, 0]
    assert pt.raw == guard[:5] + texts[0] + bytes(1) + texts[2] + guard[5 + len(ct):]
