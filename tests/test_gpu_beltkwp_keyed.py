"""-m gpu: belt-kwp with one key-encryption key per record (bee2hip_beltKWP_*keyed_batch*: the `keys` argument of
belt_kwp_batch_kernel) against the plain-Python model, record by record, every output octet compared.  tests/test_bpki.py runs the
kernel's key expansion and per-lane transform on the CPU.

The stream entry is held to the device-pointer contract the way tests/test_gpu_beltkwp.py holds its shared-key sibling: every
buffer is a slice of one allocation filled with a seeded pattern, keys, src, dst and headers at odd addresses, 4 KiB of pattern on
each side; after a call the outputs are the model's over their whole range and every other octet of the allocation is what it
was.  T is the token's size; a record to wrap has T - 16 octets."""
import ctypes
import functools
import random
import struct

import pytest
import torch

import orc_beltkwp as M
from bee2_amd import engine as E
from gpulib import engine
from test_gpu_beltkwp import Arena

pytestmark = pytest.mark.gpu
SIZES = (1, 63, 64, 65, 257)                    # 257: one record past a workgroup of four wavefronts
TOKENS = (32, 33, 47, 48, 81, 113, 1024)        # whole dwords and every residue; 81 and 113 are bpki's; the cap
KEY_LENS = (16, 24, 32)


class Batch:
    """n records under n different keys.  The unwrap input spoils every 5th record (i % 5 == 2), in turn by a flipped token
    octet and by a right token under the neighbour's key"""

    def __init__(self, T, n, key_len, seed=0):
        rnd = random.Random((T * 1000 + n) * 100 + key_len + 7919 * seed)
        self.T, self.n, self.key_len, self.count = T, n, key_len, T - 16
        self.keys = [rnd.randbytes(key_len) for _ in range(n)]
        assert len(set(self.keys)) == n
        self.hdrs = [rnd.randbytes(16) for _ in range(n)]
        self.recs = [rnd.randbytes(self.count) for _ in range(n)]
        self.tokens_clean = [M.wrap(self.recs[i], self.hdrs[i], self.keys[i]) for i in range(n)]
        self.tokens, self.refused = list(self.tokens_clean), list(range(2, n, 5))
        for i in self.refused:
            if (i // 5) % 2:
                self.tokens[i] = M.wrap(self.recs[i], self.hdrs[i], self.keys[i - 1])
            else:
                t = bytearray(self.tokens_clean[i])
                t[rnd.randrange(T)] ^= 1 << rnd.randrange(8)
                self.tokens[i] = bytes(t)
        for i in self.refused:
            assert M.unwrap(self.tokens[i], self.hdrs[i], self.keys[i]) == (M.ERR_BAD_KEYTOKEN, bytes(self.count))

    def want_unwrap(self, n):
        return (b"".join(bytes(self.count) if i in self.refused else self.recs[i] for i in range(n)),
                [M.ERR_BAD_KEYTOKEN if i in self.refused else 0 for i in range(n)])


@functools.lru_cache(maxsize=None)
def batch(T, n, key_len, seed=0):
    return Batch(T, n, key_len, seed)


def arena(b, n, unwrap, src, key_off=1, src_off=3, dst_off=5, hdr_off=7, seed=1, keys=None):
    out_len = b.count if unwrap else b.T
    A = Arena(seed).add("keys", b"".join(b.keys[:n]) if keys is None else keys, key_off).add("src", b"".join(src[:n]), src_off)
    A.add("dst", n * out_len, dst_off).add("hdrs", b"".join(b.hdrs[:n]), hdr_off)
    if unwrap:
        A.add("codes", 4 * n, 4)
    return A.build()


def run(eng, b, n, unwrap, **kw):
    """the first n records of b through the stream entry -> the output octets (and the codes)"""
    A = arena(b, n, unwrap, b.tokens if unwrap else b.recs, **kw)
    eng.beltKWP_keyed_batch_stream(unwrap, A.t("keys"), b.key_len, A.t("hdrs"), A.t("src"), b.T if unwrap else b.count, n, A.t("dst"),
                                   A.t("codes") if unwrap else None)
    got = A.fetch(["dst", "codes"] if unwrap else ["dst"])
    return (got["dst"], list(struct.unpack(f"<{n}I", got["codes"]))) if unwrap else got["dst"]


def check(eng, b, n, **kw):
    got = run(eng, b, n, 0, **kw)
    assert got == b"".join(b.tokens_clean[:n]), (b.T, n, b.key_len, "wrap", _first_bad(b.T, got, b"".join(b.tokens_clean[:n])))
    out, codes = run(eng, b, n, 1, **kw)
    want, want_codes = b.want_unwrap(n)
    assert codes == want_codes, (b.T, n, b.key_len, [i for i in range(n) if codes[i] != want_codes[i]][:8])
    assert out == want, (b.T, n, b.key_len, "unwrap", _first_bad(b.count, out, want))


def _first_bad(size, got, want):
    for i in range(len(want) // size):
        if got[size * i:size * (i + 1)] != want[size * i:size * (i + 1)]:
            return i, got[size * i:size * (i + 1)].hex(), want[size * i:size * (i + 1)].hex()


@pytest.mark.parametrize("T", TOKENS)
def test_every_batch_edge_under_a_key_per_record(T):
    """n = 1, a partial, a whole and a started second wavefront, a started second workgroup; wrap, and unwrap with every fifth
    token refused.  The key length rotates with T (the next test runs every pair)"""
    eng = engine()
    b = batch(T, 257, KEY_LENS[TOKENS.index(T) % 3])
    for n in SIZES:
        check(eng, b, n)


@pytest.mark.parametrize("key_len", KEY_LENS)
@pytest.mark.parametrize("T", TOKENS)
def test_every_key_length_at_every_token_size(T, key_len):
    """65 records; keys, src, dst and headers at 1, 3, 5, 7 mod 256 and, for the dword rows of T = 32 and 48, src and dst
    4-aligned with the keys 2 mod 4"""
    eng = engine()
    b = batch(T, 65, key_len, seed=2)
    check(eng, b, 65)
    check(eng, b, 65, key_off=2, src_off=0, dst_off=0, hdr_off=0)


def test_refused_tokens_are_zeroed_in_their_own_slot_only():
    """a flipped token octet, and a right token under the neighbour's key: ERR_BAD_KEYTOKEN and zeros there, the key elsewhere"""
    eng = engine()
    b = batch(81, 257, 32)
    out, codes = run(eng, b, 257, 1)
    assert b.refused == list(range(2, 257, 5)) and [i for i, c in enumerate(codes) if c] == b.refused
    assert {codes[i] for i in b.refused} == {E.ERR_BAD_KEYTOKEN}
    for i in range(257):
        assert out[65 * i:65 * (i + 1)] == (bytes(65) if i in b.refused else b.recs[i]), i


@pytest.mark.parametrize("T", [48, 81])
def test_equal_keys_give_what_the_shared_key_entry_gives(T):
    eng = engine()
    b = batch(T, 257, 24, seed=3)
    key = b.keys[0]
    for unwrap in (0, 1):
        # (unwrap: every 7th token is one of another key, or a spoilt one)
        src = b.recs if unwrap == 0 else [M.wrap(b.recs[i], b.hdrs[i], key) if i % 7 != 3 else b.tokens[i] for i in range(257)]
        A = arena(b, 257, unwrap, src, keys=key * 257)
        eng.beltKWP_keyed_batch_stream(unwrap, A.t("keys"), 24, A.t("hdrs"), A.t("src"), len(src[0]), 257, A.t("dst"),
                                       A.t("codes") if unwrap else None)
        outputs = ["dst", "codes"] if unwrap else ["dst"]
        keyed = A.fetch(outputs)
        A.refill()
        eng.beltKWP_batch_stream(unwrap, key, A.t("hdrs"), A.t("src"), len(src[0]), 257, A.t("dst"), A.t("codes") if unwrap else None)
        assert A.fetch(outputs) == keyed
        if unwrap:
            codes = struct.unpack("<257I", keyed["codes"])
            assert {i for i in range(257) if codes[i]} == set(range(3, 257, 7))


def test_keys_that_meet_dst_are_refused_with_nothing_written():
    eng = engine()
    A = Arena(9).add("buf", 65 * (32 + 48 + 32) + 64, 1).add("src", 65 * 48, 3).build()
    s, _ = A.at["buf"]
    codes = torch.zeros(65, dtype=torch.int32, device="cuda")
    for unwrap, count, dst_len in ((0, 32, 65 * 48), (1, 48, 65 * 32)):
        for key_at, dst_at in ((0, 0), (0, 65 * 32 - 1), (dst_len - 1, 0), (8, 0)):
            with pytest.raises(E.EngineError):
                eng.beltKWP_keyed_batch_stream(unwrap, A.dev[s + key_at:s + key_at + 65 * 32], 32, None, A.t("src")[:65 * count], count, 65,
                                               A.dev[s + dst_at:s + dst_at + dst_len], codes)
    assert A.fetch([]) == {} and not codes.any()


def test_host_entries_with_dst_equal_to_src():
    """bee2hip_beltKWP_wrap_keyed_batch / _unwrap_keyed_batch once each, in place, refused tokens among them"""
    eng = engine()
    b = batch(49, 65, 24, seed=4)
    _sz = ctypes.c_size_t
    keys, hdrs = b"".join(b.keys), b"".join(b.hdrs)
    buf = ctypes.create_string_buffer(b"".join(b.recs), 65 * b.T)
    assert eng.lib.bee2hip_beltKWP_wrap_keyed_batch(keys, _sz(24), hdrs, buf, _sz(33), _sz(65), buf) == E.ERR_OK
    assert buf.raw == b"".join(b.tokens_clean)
    tokens = b"".join(b.tokens)
    buf = ctypes.create_string_buffer(tokens, 65 * b.T)
    codes = (ctypes.c_uint32 * 65)()
    assert eng.lib.bee2hip_beltKWP_unwrap_keyed_batch(keys, _sz(24), hdrs, buf, _sz(b.T), _sz(65), buf, codes) == E.ERR_OK
    want, want_codes = b.want_unwrap(65)
    assert buf.raw[:65 * 33] == want and list(codes) == want_codes and buf.raw[65 * 33:] == tokens[65 * 33:]
    assert eng.beltKWP_wrap_keyed_batch(keys, 24, None, b"".join(b.recs), 33) == \
        (E.ERR_OK, b"".join(M.wrap(b.recs[i], None, b.keys[i]) for i in range(65)))
    assert eng.beltKWP_unwrap_keyed_batch(keys, 24, hdrs, tokens, b.T) == (E.ERR_OK, want, want_codes)
