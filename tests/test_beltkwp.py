"""CPU side of belt-kwp (key wrap, STB 34.101.31): the plain-Python model (tests/orc_beltkwp.py) against the reference's recorded
outputs and the standard's vectors A.21 / A.22; the kernel's own per-lane transform and launch plan
(bee2_amd/csrc/belt_kwp_common.hpp) against the model through a g++ shim, for every token size the entries accept; the three
names in the header, the library and the engine; every refusal of the C ABI without a device."""
import ctypes
import json
import os
import random
import re
import subprocess

import pytest

import bee2_amd
import beltkwpgrid as G
import orc_beltkwp as M
from bee2_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "hostshim")
NAMES = ("bee2hip_beltKWP_wrap_batch", "bee2hip_beltKWP_unwrap_batch", "bee2hip_beltKWP_batch_stream")
_sz, _u32 = ctypes.c_size_t, ctypes.c_uint32


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "belt_kwp.json")))


# ================================================================================================ the model
def test_fixture_covers_every_count_key_length_and_header_form(fixture):
    rows = fixture["rows"]
    assert [{k: r[k] for k in ("count", "key_len", "header", "seed")} for r in rows] == G.fixture_cases()
    assert {r["count"] for r in rows} == set(range(16, 100)) | {127, 128, 129, 1007, 1008} | {288, 289, 592, 593}
    assert G.FIXTURE_COUNTS[-4:] == [288, 289, 592, 593] and set(G.FIXTURE_COUNTS[-4:]) <= set(G.SEAM_COUNTS)
    for count in G.FIXTURE_COUNTS:
        mine = [r for r in rows if r["count"] == count]
        assert {(r["key_len"], r["header"]) for r in mine} == {(k, h) for k in G.KEY_LENS for h in (True, False)}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "belt_kwp.json")) < 300 * 1024


def test_model_reproduces_every_fixture_row(fixture):
    for r in fixture["rows"]:
        x = G.case_inputs(r)
        token = M.wrap(x["src"], x["header"], x["key"])
        assert G.encode(token) == r["token"], r
        assert M.unwrap(token, x["header"], x["key"]) == (M.ERR_OK, x["src"])
        code, out = M.unwrap(G.flipped(token, x["flip"]), x["header"], x["key"])
        assert (code, G.encode(out)) == (r["flip_code"], r["flip_out"]) and code == M.ERR_BAD_KEYTOKEN and not any(out), r
        code, out = M.unwrap(token, x["wrong_header"], x["key"])
        assert (code, G.encode(out)) == (r["hdr_code"], r["hdr_out"]) and code == M.ERR_BAD_KEYTOKEN and not any(out), r


def test_model_reproduces_the_published_vectors(fixture, golden):
    """STB 34.101.31 A.21 and A.22 (test/crypto/belt_test.c:565-592 of the reference)"""
    H = golden.H
    a21 = bytes.fromhex("49A38EE108D6C742E52B774F00A6EF98B106CBD13EA4FB0680323051BC04DF76E487B055C69BCF541176169F1DC9F6C8")
    assert fixture["a21"]["token"] == a21.hex()
    assert M.wrap(H[:32], H[32:48], H[128:160]) == a21
    assert M.unwrap(a21, H[32:48], H[128:160]) == (M.ERR_OK, H[:32])
    key22 = bytes.fromhex("92632EE0C21AD9E09A39343E5C07DAA4889B03F2E6847EB152EC99F7A4D9F154")
    hdr22 = bytes.fromhex("B5EF68D8E4A39E567153DE13D72254EE")
    assert fixture["a22"] == {"key": key22.hex(), "header": hdr22.hex()}
    assert M.wbl_decr(H[64:112], H[160:192]) == key22 + hdr22
    assert M.unwrap(H[64:112], hdr22, H[160:192]) == (M.ERR_OK, key22)


@pytest.mark.ref
def test_model_equals_the_live_reference_on_a_fresh_seed():
    import refgen
    if not refgen.have_ref():
        pytest.skip("oracle/_ref not built")
    L = refgen.ref()
    seed = int.from_bytes(os.urandom(4), "little")               # random.Random(seed) below reproduces a failure
    print("seed", seed)
    rnd = random.Random(seed)
    for count in G.FIXTURE_COUNTS:
        key, hdr, src = rnd.randbytes(rnd.choice(G.KEY_LENS)), rnd.choice((None, rnd.randbytes(16))), rnd.randbytes(count)
        dst = ctypes.create_string_buffer(count + 16)
        assert L.beltKWPWrap(dst, src, _sz(count), hdr, key, _sz(len(key))) == 0
        assert dst.raw == M.wrap(src, hdr, key), (seed, count, key, hdr, src)
        tok = G.flipped(dst.raw, (rnd.randrange(count + 16), rnd.randrange(8)))
        back = ctypes.create_string_buffer(count)
        code = L.beltKWPUnwrap(back, tok, _sz(count + 16), hdr, key, _sz(len(key)))
        assert (code, back.raw) == M.unwrap(tok, hdr, key), (seed, count, key, hdr, tok)


# ================================================================================================ the kernel's transform
@pytest.fixture(scope="module")
def hk(tmp_path_factory, golden):
    out = tmp_path_factory.mktemp("hostkwp") / "libhostkwp.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", "-o", str(out),
                           os.path.join(SHIM, "host_kwp_shim.cpp")])
    lib = ctypes.CDLL(str(out))
    for name in ("hk_lane", "hk_pad", "hk_dwords"):
        getattr(lib, name).restype = _u32
    lib.hk_init(golden.H)
    return lib


def _lane(hk, orc, unwrap, T, key, hdr, data, lane, seed):
    out = ctypes.create_string_buffer(T - 16 if unwrap else T)
    code = hk.hk_lane(unwrap, _u32(T), orc.key_expand(key), hdr, bytes(data), out, _u32(lane), _u32(seed))
    return code, out.raw


def test_transform_equals_the_model_for_every_count_in_both_directions(hk, orc):
    """kwp_lane() of belt_kwp_common.hpp -- the text the kernel runs -- in one column of a [dword][64] array whose other
    octets hold a pattern (the shim answers 0xFFFFFFFF when one of them changes): every wrap count 16 .. 1008, hence every
    T mod 16, every tail residue and every trip count, wrapped, unwrapped, and unwrapped after a token bit and after a header
    bit was flipped.  Key lengths, header / NULL header and the lane rotate"""
    rnd = random.Random(0x4B5750)
    for count in range(16, 1009):
        T = count + 16
        key = rnd.randbytes(G.KEY_LENS[count % 3])
        hdr = rnd.randbytes(16) if count % 4 else None
        src, lane = rnd.randbytes(count), rnd.randrange(64)
        token = M.wrap(src, hdr, key)
        assert _lane(hk, orc, 0, T, key, hdr, src, lane, count) == (M.ERR_OK, token), count
        assert _lane(hk, orc, 1, T, key, hdr, token, 63 - lane, count) == (M.ERR_OK, src), count
        spoilt = G.flipped(token, (rnd.randrange(T), rnd.randrange(8)))
        want = M.unwrap(spoilt, hdr, key)
        assert want == (M.ERR_BAD_KEYTOKEN, bytes(count))
        assert _lane(hk, orc, 1, T, key, hdr, spoilt, lane, count + 1) == want, count
        wrong = G.flipped(hdr or bytes(16), (rnd.randrange(16), rnd.randrange(8)))
        assert _lane(hk, orc, 1, T, key, wrong, token, lane, count + 2) == want, count
        if hdr is not None:                                       # a NULL header against a nonzero one
            assert _lane(hk, orc, 1, T, key, None, token, lane, count + 3) == want, count


def test_transform_on_the_published_vectors(hk, orc, golden):
    H = golden.H
    a21 = bytes.fromhex("49A38EE108D6C742E52B774F00A6EF98B106CBD13EA4FB0680323051BC04DF76E487B055C69BCF541176169F1DC9F6C8")
    assert _lane(hk, orc, 0, 48, H[128:160], H[32:48], H[:32], 1, 1) == (0, a21)
    assert _lane(hk, orc, 1, 48, H[128:160], H[32:48], a21, 1, 2) == (0, H[:32])
    hdr22 = bytes.fromhex("B5EF68D8E4A39E567153DE13D72254EE")
    assert _lane(hk, orc, 1, 48, H[160:192], hdr22, H[64:112], 0, 3) == \
        (0, bytes.fromhex("92632EE0C21AD9E09A39343E5C07DAA4889B03F2E6847EB152EC99F7A4D9F154"))


def test_slab_layout_and_launch_plan(hk):
    """a token ends with its column's last dword; a wavefront owns 256 ceil(T / 4) octets; a workgroup never exceeds 80 KiB
    (two fit a CU's 160 KiB), holds 4, 2 or 1 wavefronts, as many as fit, and one at the cap"""
    plan = (_u32 * 3)()
    seen = set()
    for T in range(32, 1025):
        assert (hk.hk_pad(_u32(T)) + T) % 4 == 0 and hk.hk_pad(_u32(T)) < 4 and hk.hk_dwords(_u32(T)) == -(-T // 4)
        hk.hk_plan(_u32(T), plan)
        waves, wave_bytes, lds = plan
        assert wave_bytes == 256 * -(-T // 4) and lds == 4096 + waves * wave_bytes
        assert waves in (1, 2, 4) and lds <= 80 * 1024
        assert waves == 4 or 4096 + 2 * waves * wave_bytes > 80 * 1024
        assert (waves, lds) == G.plan(T)                          # the restatement the GPU seam tests compute their plans with
        assert waves == (4 if T <= 304 else 2 if T <= 608 else 1)
        seen.add(waves)
    assert seen == {1, 2, 4} and waves == 1 and lds == 4096 + 65536
    # the seam counts of the GPU tests sit on both sides of both changes, and reach the 80 KiB launch of either form
    plans = [G.plan(c + 16) for c in G.SEAM_COUNTS]
    assert [w for w, _ in plans] == [4, 4, 2, 2, 2, 2, 1, 1] and {w for w, lds in plans if lds == 81920} == {2, 4}


# ================================================================================================ the interface
def test_header_exports_and_engine_list_the_three_names():
    header = open(os.path.join(ROOT, "include", "bee2hip.h")).read()
    exported = E.lib_exports()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in exported, name
        assert name in E.BATCH_SYMBOLS, name
    assert {"beltKWP_wrap_batch", "beltKWP_unwrap_batch", "beltKWP_batch_stream"} <= set(dir(E.Engine))
    assert re.search(r"#define ERR_BAD_KEYTOKEN\s+\(\(err_t\)513\)", header) and E.ERR_BAD_KEYTOKEN == 513 == M.ERR_BAD_KEYTOKEN
    # bee2's own names stay out: a single token is one serial chain (tests/test_gpu_reftests.py says "not a drop-in symbol")
    assert not [n for n in exported if n.startswith("beltKWP")]


def test_every_refusal_answers_without_a_device():
    """(this machine may have no GPU at all: an entry that reached for the device would answer ERR_BEE2HIP_DEVICE)"""
    lib = bee2_amd.load().lib
    key, buf, codes = bytes(32), ctypes.create_string_buffer(4096), (_u32 * 4)()
    fake = ctypes.c_void_p(0x10000)                        # never dereferenced: every call below is refused first

    def wrap(key=key, key_len=32, count=32, n=1, src=buf, dst=buf):
        return lib.bee2hip_beltKWP_wrap_batch(key, _sz(key_len), None, src, _sz(count), _sz(n), dst)

    def unwrap(key=key, key_len=32, count=48, n=1, src=buf, dst=buf, codes=codes):
        return lib.bee2hip_beltKWP_unwrap_batch(key, _sz(key_len), None, src, _sz(count), _sz(n), dst, codes)

    def stream(unwrap=0, key=key, key_len=32, count=48, n=1, src=fake, dst=ctypes.c_void_p(0x20000), codes=ctypes.c_void_p(0x30000)):
        return lib.bee2hip_beltKWP_batch_stream(ctypes.c_int(unwrap), key, _sz(key_len), None, src, _sz(count), _sz(n), dst, codes, None)

    def swrap(**kw):
        return stream(unwrap=0, **kw)

    def sunwrap(**kw):
        return stream(unwrap=1, **kw)

    for f, lo, hi in ((wrap, 16, 1008), (swrap, 16, 1008), (unwrap, 32, 1024), (sunwrap, 32, 1024)):
        assert f(count=lo - 1) == f(count=0) == f(count=lo - 1, n=0) == E.ERR_BAD_INPUT
        assert f(key_len=0) == f(key_len=17) == f(key_len=33) == f(key=None) == E.ERR_BAD_INPUT
        assert f(n=1 << 32) == E.ERR_BAD_INPUT
        assert f(count=hi + 1) == f(count=hi + 1, n=0) == f(count=1 << 40) == E.ERR_NOT_IMPLEMENTED
        assert f(count=hi + 1, key_len=20) == E.ERR_BAD_INPUT      # bad input before not implemented
        assert f(src=None) == f(dst=None) == E.ERR_BAD_INPUT
        assert f(n=0) == f(n=0, src=None, dst=None) == f(n=0, count=lo) == f(n=0, count=hi) == E.ERR_OK
    assert unwrap(codes=None) == sunwrap(codes=None) == E.ERR_BAD_INPUT
    assert unwrap(codes=None, n=0) == sunwrap(codes=None, n=0) == E.ERR_OK
    # the stream entry: the direction, the alignment of the codes, and any overlap of the two ranges
    assert stream(unwrap=2) == stream(unwrap=-1) == E.ERR_BAD_INPUT
    assert sunwrap(codes=ctypes.c_void_p(0x30002)) == E.ERR_BAD_INPUT
    s = 0x10000
    for unw, count, out in ((0, 32, 48), (1, 48, 32)):
        for d in (s, s + 1, s + 4 * count - 1, s - 4 * out + 1, s - 1):
            assert stream(unwrap=unw, count=count, n=4, src=ctypes.c_void_p(s), dst=ctypes.c_void_p(d)) == E.ERR_BAD_INPUT, (unw, d - s)
