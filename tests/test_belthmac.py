"""CPU side of belt-hmac / belt-pbkdf2 (STB 34.101.31): the model (tests/orc_belthmac.py, compositions of the oracle's belt-hash)
against the reference's recorded outputs and the published vectors; the kernel's own per-lane logic
(bee2_amd/csrc/belt_hmac_common.hpp) and the host path of the one-shots (host_hmac.hpp) against the model through a g++ shim,
for every key length 0..100 x message length 0..100; the names in the header, the library and the engine; every refusal of the
C ABI without a device."""
import ctypes
import json
import os
import random
import re
import subprocess

import pytest

import bee2_amd
import belthmacgrid as G
import orc_belthmac as M
from bee2_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "hostshim")
BATCH_NAMES = ("bee2hip_beltHMAC_ragged", "bee2hip_beltHMAC_verify_ragged", "bee2hip_beltHMAC_ragged_stream",
               "bee2hip_beltPBKDF2_batch", "bee2hip_beltPBKDF2_batch_stream")
DROPIN_NAMES = ("beltHMAC", "beltPBKDF2")
_sz, _u32, _u64 = ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "belt_hmac.json")))


def model(c, key, msg):
    return M.hmac(key, msg) if c["kind"] == "hmac" else M.pbkdf2(key, c["iter"], msg)


# ================================================================================================ the model
def test_fixture_covers_every_key_length_message_length_and_iteration_count(fixture):
    rows = fixture["rows"]
    assert [{k: r[k] for k in ("kind", "key_len", "msg_len", "iter", "seed")} for r in rows] == G.fixture_cases()
    assert {(r["key_len"], r["msg_len"]) for r in rows if r["kind"] == "hmac"} == {(k, m) for k in G.KEY_LENS for m in G.MSG_LENS}
    assert {(r["key_len"], r["msg_len"], r["iter"]) for r in rows if r["kind"] == "pbkdf2"} == \
        {(k, m, i) for k in G.KEY_LENS for m in G.MSG_LENS for i in G.ITERS}
    assert G.KEY_LENS == (0, 1, 29, 31, 32, 33, 42, 63, 64, 65, 97)
    assert G.MSG_LENS == (0, 1, 27, 28, 29, 31, 32, 33, 63, 64, 65, 100, 1000) and G.ITERS == (1, 2, 3, 50)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "belt_hmac.json")) < 200 * 1024


def test_model_reproduces_every_fixture_row(fixture):
    for r in fixture["rows"]:
        key, msg = G.case_inputs(r)
        assert model(r, key, msg).hex() == r["out"], r


def test_model_reproduces_the_published_vectors(fixture, golden):
    """STB 34.101.31 B.1-1 .. B.1-3 (test/crypto/belt_test.c:787-819 of the reference) and the PBKDF2 vectors of
    test/crypto/bign_test.c:521-553"""
    H = golden.H
    want = {29: "D4828E6312B08BB83C9FA6535A4635549E411FD11C0D8289359A1130E930676B"}
    for v in fixture["b1"]:
        assert M.hmac(H[128:128 + v["key_len"]], H[192:224]).hex() == v["mac"]
        assert v["mac"].upper() == want.get(v["key_len"], v["mac"].upper())
    assert [v["key_len"] for v in fixture["b1"]] == [29, 32, 42]
    keys = ["3D331BBBB1FBBB40E4BF22F6CB9A689EF13A77DC09ECF93291BFE42439A72E7D",
            "7249B4785FE68B1586D189A23E3842E48705C080A3248D8F0E8C3D63A93B2670",
            "E48329259BC1211DDAC2EF1DADFFC9932702A92F1DD66C14A9BA1D7300C8713C"]
    assert [v["key"].upper() for v in fixture["pbkdf2"]] == keys
    assert fixture["pbkdf2"][0]["salt"] == H[192:200].hex() and fixture["pbkdf2"][0]["pwd"] == "B194BAC80A08F53B"
    v = fixture["pbkdf2"][1]                                         # 2048 iterations; the 10 000 ones run in the shim below
    assert M.pbkdf2(v["pwd"].encode(), v["iter"], bytes.fromhex(v["salt"])).hex() == v["key"]


@pytest.mark.ref
def test_model_equals_the_live_reference_on_a_fresh_seed():
    import refgen
    if not refgen.have_ref():
        pytest.skip("oracle/_ref not built")
    L = refgen.ref()
    seed = int.from_bytes(os.urandom(4), "little")               # random.Random(seed) below reproduces a failure
    print("seed", seed)
    rnd = random.Random(seed)
    out = ctypes.create_string_buffer(32)
    for _ in range(200):
        key, msg, it = rnd.randbytes(rnd.randrange(130)), rnd.randbytes(rnd.randrange(200)), rnd.randrange(1, 6)
        assert L.beltHMAC(out, msg, _sz(len(msg)), key, _sz(len(key))) == 0
        assert out.raw == M.hmac(key, msg), (seed, key, msg)
        assert L.beltPBKDF2(out, key, _sz(len(key)), _sz(it), msg, _sz(len(msg))) == 0
        assert out.raw == M.pbkdf2(key, it, msg), (seed, key, it, msg)


# ================================================================================================ the kernel's lane logic
@pytest.fixture(scope="module")
def hh(tmp_path_factory, golden):
    out = tmp_path_factory.mktemp("hosthmac") / "libhosthmac.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-o", str(out),
                           os.path.join(SHIM, "host_hmac_shim.cpp")])
    lib = ctypes.CDLL(str(out))
    lib.hh_lane.restype = lib.hh_differs.restype = _u32
    lib.hh_init(golden.H)
    return lib


def lane(hh, shared, key, msg, suffix, it, seed=1):
    """hmac_lane() through a reader that leaves a pattern behind the octets asked for and counts a read past the record"""
    out = ctypes.create_string_buffer(32)
    faults = hh.hh_lane(_u32(shared), bytes(key), _u64(len(key)), bytes(msg), _u64(len(msg)), _u32(suffix), _u32(it), _u32(seed), out)
    assert faults == 0, (len(key), len(msg), suffix, it)
    return out.raw


def host(hh, key, msg, suffix, it):
    out = ctypes.create_string_buffer(32)
    hh.hh_host(bytes(key), _u64(len(key)), bytes(msg), _u64(len(msg)), _u32(suffix), _u32(it), out)
    return out.raw


def test_lane_equals_the_model_for_every_key_and_message_length(hh):
    """every key length 0..100 x message length 0..100 -- zero-padded and hashed keys, every tail residue, the empty message --
    as HMAC (iter 1) and with two further rounds (iter 3, no suffix: the XOR of t1, t2, t3); the key per record and, every third
    case, as the launch's shared state"""
    rnd = random.Random(0x484D4143)
    for klen in range(101):
        key = rnd.randbytes(klen)
        for mlen in range(101):
            msg = rnd.randbytes(mlen)
            t1 = M.hmac(key, msg)
            shared = (klen + mlen) % 3 == 0
            assert lane(hh, shared, key, msg, 0, 1, klen * 101 + mlen) == t1, (klen, mlen)
            t2 = M.hmac(key, t1)
            t3 = M.hmac(key, t2)
            want = bytes(a ^ b ^ c for a, b, c in zip(t1, t2, t3))
            assert lane(hh, not shared, key, msg, 0, 3, klen + mlen) == want, (klen, mlen)


def test_lane_equals_the_model_for_every_salt_length_with_the_suffix(hh):
    """salt lengths 0..70: the suffix 00 00 00 01 inside a block, filling it exactly (28 mod 32), straddling two (29, 30, 31),
    starting one (0 mod 32); iter 1, 2 and 50; passwords short and hashed"""
    rnd = random.Random(0x50424B44)
    for slen in range(71):
        salt = rnd.randbytes(slen)
        for it in (1, 2, 50):
            pwd = rnd.randbytes(G.KEY_LENS[(slen + it) % len(G.KEY_LENS)])
            assert lane(hh, slen % 2, pwd, salt, 4, it, slen) == M.pbkdf2(pwd, it, salt), (slen, it)


def test_lane_and_host_path_on_the_published_vectors(hh, fixture, golden):
    H = golden.H
    for v in fixture["b1"]:
        for shared in (0, 1):
            assert lane(hh, shared, H[128:128 + v["key_len"]], H[192:224], 0, 1).hex() == v["mac"]
        assert host(hh, H[128:128 + v["key_len"]], H[192:224], 0, 1).hex() == v["mac"]
    for v in fixture["pbkdf2"]:
        assert lane(hh, 0, v["pwd"].encode(), bytes.fromhex(v["salt"]), 4, v["iter"]).hex() == v["key"]
        assert host(hh, v["pwd"].encode(), bytes.fromhex(v["salt"]), 4, v["iter"]).hex() == v["key"]


def test_host_path_of_the_one_shots_equals_the_fixture(hh, fixture):
    """hmac_run() of host_hmac.hpp, what beltHMAC and beltPBKDF2 run on the host"""
    for r in fixture["rows"]:
        key, msg = G.case_inputs(r)
        assert host(hh, key, msg, 0 if r["kind"] == "hmac" else 4, r["iter"]).hex() == r["out"], r


def test_comparison_looks_at_the_first_mac_len_octets_only(hh):
    rnd = random.Random(5)
    a = rnd.randbytes(32)
    for mac_len in range(1, 33):
        assert hh.hh_differs(a, a, _u32(mac_len)) == 0
        for octet in range(32):
            for bit in (0, 7):
                b = bytearray(a)
                b[octet] ^= 1 << bit
                assert hh.hh_differs(a, bytes(b), _u32(mac_len)) == (1 if octet < mac_len else 0), (mac_len, octet, bit)


# ================================================================================================ the interface
def test_header_exports_and_engine_list_the_names():
    header = open(os.path.join(ROOT, "include", "bee2hip.h")).read()
    exported = E.lib_exports()
    for name in BATCH_NAMES + DROPIN_NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in exported, name
        assert name in (E.BATCH_SYMBOLS if name in BATCH_NAMES else E.DROPIN_SYMBOLS), name
    text = open(os.path.join(ROOT, "bee2_amd", "csrc", "exports.map")).read()
    assert "bee2hip_*;" in text and "belt*;" in text
    assert {"beltHMAC_ragged", "beltHMAC_verify_ragged", "beltHMAC_ragged_stream", "beltPBKDF2_batch", "beltPBKDF2_batch_stream",
            "beltHMAC", "beltPBKDF2"} <= set(dir(E.Engine))
    assert E.ERR_BAD_MAC == 511 == M.ERR_BAD_MAC
    # bee2's step functions stay out
    assert not [n for n in exported if n.startswith("beltHMAC") and n != "beltHMAC"]


def test_every_refusal_answers_without_a_device():
    """(this machine may have no GPU at all: an entry that reached for the device would answer ERR_BEE2HIP_DEVICE)"""
    lib = bee2_amd.load().lib
    key, buf, codes = bytes(32), ctypes.create_string_buffer(4096), (_u32 * 4)()
    offs = (_u64 * 3)(0, 10, 20)
    down = (_u64 * 3)(0, 10, 5)
    fake = [ctypes.c_void_p(0x10000 * (k + 1)) for k in range(8)]       # never dereferenced: every call below is refused first
    BAD, NOT, OK = E.ERR_BAD_INPUT, E.ERR_NOT_IMPLEMENTED, E.ERR_OK

    def mac(key=key, key_len=32, keys=None, koffs=None, data=buf, offs=offs, n=2, macs=buf, mac_len=32):
        return lib.bee2hip_beltHMAC_ragged(key, _sz(key_len), keys, koffs, data, offs, _sz(n), macs, _sz(mac_len))

    def vfy(key=key, key_len=32, keys=None, koffs=None, data=buf, offs=offs, n=2, macs=buf, mac_len=32, codes=codes):
        return lib.bee2hip_beltHMAC_verify_ragged(key, _sz(key_len), keys, koffs, data, offs, _sz(n), macs, _sz(mac_len), codes)

    def smac(verify=0, key=key, key_len=32, keys=None, koffs=None, data=fake[0], offs=fake[1], order=None, n=2, macs=fake[2],
             mac_len=32, codes=None):
        return lib.bee2hip_beltHMAC_ragged_stream(ctypes.c_int(verify), key, _sz(key_len), keys, koffs, data, offs, order, _sz(n),
                                                  macs, _sz(mac_len), codes, None)

    def svfy(**kw):
        kw.setdefault("codes", fake[3])
        return smac(verify=1, **kw)

    for f in (mac, vfy, smac, svfy):
        assert f(mac_len=0) == f(mac_len=33) == f(mac_len=0, n=0) == f(mac_len=1 << 40) == BAD
        assert f(n=1 << 32) == BAD
        assert f(keys=buf if f in (mac, vfy) else fake[4], koffs=offs if f in (mac, vfy) else fake[5]) == BAD       # both forms
        assert f(key=None) == BAD                                                                                 # neither
        assert f(offs=None) == f(macs=None) == BAD
        assert f(n=0) == f(n=0, offs=None, macs=None, data=None) == f(n=0, key=None) == OK
        assert f(key=None, keys=buf if f in (mac, vfy) else fake[4]) == BAD                  # keys without their offsets
    assert vfy(codes=None) == svfy(codes=None) == BAD and vfy(codes=None, n=0) == svfy(codes=None, n=0) == OK
    assert mac(offs=down) == vfy(offs=down) == mac(key=None, keys=buf, koffs=down) == BAD
    assert mac(data=None) == vfy(data=None) == mac(key=None, keys=None, koffs=offs) == BAD
    assert smac(verify=2) == smac(verify=-1) == BAD
    odd = ctypes.c_void_p(0x10004)
    assert smac(offs=odd) == smac(key=None, keys=fake[4], koffs=odd) == smac(order=ctypes.c_void_p(0x10002)) == BAD
    assert svfy(codes=ctypes.c_void_p(0x30002)) == BAD

    poffs = (_u64 * 3)(0, 3, 9)

    def kdf(pwds=buf, poffs=poffs, iters=2, salts=buf, salt_len=8, stride=8, n=2, keys=buf):
        return lib.bee2hip_beltPBKDF2_batch(pwds, poffs, _sz(iters), salts, _sz(salt_len), _sz(stride), _sz(n), keys)

    def skdf(pwds=fake[0], poffs=fake[1], iters=2, salts=fake[2], salt_len=8, stride=8, order=None, n=2, keys=fake[3]):
        return lib.bee2hip_beltPBKDF2_batch_stream(pwds, poffs, _sz(iters), salts, _sz(salt_len), _sz(stride), order, _sz(n), keys, None)

    for f in (kdf, skdf):
        assert f(iters=0) == f(iters=0, n=0) == BAD
        assert f(n=1 << 32) == BAD
        assert f(stride=7) == f(stride=1) == f(stride=7, n=0) == BAD
        assert f(iters=G.ITER_CAP + 1) == f(iters=1 << 40) == f(iters=G.ITER_CAP + 1, n=0) == NOT
        assert f(iters=G.ITER_CAP + 1, stride=3) == BAD               # bad input before not implemented
        assert f(poffs=None) == f(keys=None) == f(salts=None) == BAD
        assert f(n=0) == f(n=0, poffs=None, keys=None, salts=None, pwds=None) == f(n=0, iters=G.ITER_CAP) == f(n=0, stride=0) == OK
    assert kdf(poffs=down) == kdf(pwds=None) == BAD
    assert skdf(poffs=ctypes.c_void_p(0x10004)) == skdf(order=ctypes.c_void_p(0x10002)) == BAD

    # the one-shots: what bee2 refuses (belt_hmac.c:249-252, belt_pbkdf.c:32-36)
    out = ctypes.create_string_buffer(32)
    assert lib.beltHMAC(None, buf, _sz(4), key, _sz(32)) == lib.beltHMAC(out, None, _sz(4), key, _sz(32)) == BAD
    assert lib.beltHMAC(out, buf, _sz(4), None, _sz(32)) == BAD
    assert lib.beltPBKDF2(out, key, _sz(8), _sz(0), buf, _sz(8)) == lib.beltPBKDF2(None, key, _sz(8), _sz(1), buf, _sz(8)) == BAD
    assert lib.beltPBKDF2(out, None, _sz(8), _sz(1), buf, _sz(8)) == lib.beltPBKDF2(out, key, _sz(8), _sz(1), None, _sz(8)) == BAD
