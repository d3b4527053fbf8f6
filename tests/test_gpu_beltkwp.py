"""-m gpu: the belt-kwp batch (bee2hip_beltKWP_*batch*, bee2_amd/csrc/belt_kwp_kernels.hip) against the plain-Python model, record
by record, every output octet compared (tests/beltkwpgrid.py builds the batches; tests/test_beltkwp.py pins the model to the
reference and the kernel's per-lane transform to the model on the CPU).

The stream entry is a device-pointer batch entry that is not in the contract registry of tests/devcontract.py, so this file
holds it to the same contract itself, as tests/test_gpu_beltfmt.py does: every buffer is a slice of one allocation filled with a
seeded pattern, at the weakest alignment the header grants, with 4 KiB of pattern on each side; after a call the outputs are
the model's over their whole range and every other octet of the allocation -- inputs and guards -- is what it was.  A `count`
below is always the WRAP count; the token has count + 16 octets."""
import ctypes
import random
import struct

import numpy as np
import pytest
import torch

import beltkwpgrid as G
import orc_beltkwp as M
import orclib
from bee2_amd import engine as E
from gpulib import engine

pytestmark = pytest.mark.gpu
GUARD = 4096


class Arena:
    """named buffers inside one device allocation of seeded pattern, GUARD octets of it around each"""

    def __init__(self, seed):
        self.seed, self.at, self.data, self.pos = seed, {}, {}, GUARD

    def add(self, name, data, off=0):
        """`data` at an address = off mod 256 (a length: that many octets of pattern)"""
        start = (self.pos + 255) // 256 * 256 + off
        n = data if isinstance(data, int) else len(data)
        self.at[name], self.pos = (start, n), start + n + GUARD
        if not isinstance(data, int):
            self.data[name] = bytes(data)
        return self

    def build(self):
        self.image = np.frombuffer(random.Random(self.seed).randbytes(self.pos), dtype=np.uint8).copy()
        for name, d in self.data.items():
            self.put(name, d)
        self.dev = torch.from_numpy(self.image).cuda()
        assert self.dev.data_ptr() % 256 == 0
        return self

    def put(self, name, d):
        s, n = self.at[name]
        assert len(d) == n
        self.image[s:s + n] = np.frombuffer(bytes(d), dtype=np.uint8)

    def refill(self):
        self.dev.copy_(torch.from_numpy(self.image))
        torch.cuda.synchronize()

    def t(self, name):
        s, n = self.at[name]
        return self.dev[s:s + n]

    def fetch(self, outputs):
        """-> {name: bytes} of the outputs, after checking that nothing else changed"""
        torch.cuda.synchronize()
        got = self.dev.cpu().numpy()
        mask = np.ones(self.pos, dtype=bool)
        for name in outputs:
            s, n = self.at[name]
            mask[s:s + n] = False
        bad = np.nonzero((got != self.image) & mask)[0]
        assert bad.size == 0, f"{bad.size} octets outside the outputs changed, first at {int(bad[0])}: {self.at}"
        return {name: got[self.at[name][0]:self.at[name][0] + self.at[name][1]].tobytes() for name in outputs}


def arena(b, unwrap, src, src_off=1, dst_off=3, hdr_off=5, seed=1):
    """src, dst and the headers at odd addresses unless told otherwise; the codes (unwrap) start 4 mod 8"""
    out_len = b.count if unwrap else b.T
    A = Arena(seed).add("src", src, src_off).add("dst", b.n * out_len, dst_off)
    if b.hdrs is not None:
        A.add("hdrs", b.hdrs, hdr_off)
    if unwrap:
        A.add("codes", 4 * b.n, 4)
    return A.build()


def call(eng, b, A, unwrap):
    eng.beltKWP_batch_stream(unwrap, b.key, A.t("hdrs") if "hdrs" in A.at else None, A.t("src"), b.T if unwrap else b.count, b.n,
                             A.t("dst"), A.t("codes") if unwrap else None)


def run_wrap(eng, b, **kw):
    A = arena(b, 0, b.keys, **kw)
    call(eng, b, A, 0)
    return A.fetch(["dst"])["dst"]


def run_unwrap(eng, b, tokens, **kw):
    """-> (the output octets, [codes])"""
    A = arena(b, 1, tokens, **kw)
    call(eng, b, A, 1)
    got = A.fetch(["dst", "codes"])
    return got["dst"], list(struct.unpack(f"<{b.n}I", got["codes"]))


def check(eng, b, **kw):
    """both directions of batch b against the model"""
    got = run_wrap(eng, b, **kw)
    assert got == b.tokens_clean, (b.count, b.n, "wrap", _first_bad(b.T, got, b.tokens_clean))
    out, codes = run_unwrap(eng, b, b.tokens, **kw)
    want, want_codes = b.want_unwrap()
    assert codes == want_codes, (b.count, b.n, [i for i in range(b.n) if codes[i] != want_codes[i]][:8])
    assert out == want, (b.count, b.n, "unwrap", _first_bad(b.count, out, want))


def _first_bad(size, got, want):
    for i in range(len(want) // size):
        if got[size * i:size * (i + 1)] != want[size * i:size * (i + 1)]:
            return i, got[size * i:size * (i + 1)].hex(), want[size * i:size * (i + 1)].hex()


# ================================================================================================ shapes
@pytest.mark.parametrize("count", G.GPU_COUNTS)
def test_counts_at_every_batch_edge(count):
    """T = 32 (the sum is r1 alone), every tail residue mod 4, a dword tail that is not a multiple of 8, T = 40 (8 mod 16), around
    the A.21 shape, around four whole blocks, T = 256; n = 1, a partial, a whole and a started second wavefront, a started
    second workgroup.  Key lengths and headers / NULL headers rotate"""
    eng = engine()
    for j, n in enumerate(G.BATCH_SIZES):
        k = j + G.GPU_COUNTS.index(count)
        check(eng, G.batch(count, n, G.KEY_LENS[k % 3], hdrs=k % 4 != 1))


@pytest.mark.parametrize("count", G.GPU_COUNTS_CAP)
def test_counts_at_the_cap(count):
    """T = 1023 and 1024: 64 KiB of slab, one wavefront per workgroup, two workgroups started"""
    check(engine(), G.batch(count, 65, G.KEY_LENS[count % 3]))


@pytest.mark.parametrize("count", G.SEAM_COUNTS)
def test_both_sides_of_both_seams_of_the_launch_plan(count):
    """the launcher picks 4, 2 or 1 wavefronts per workgroup from T (kwp_plan, belt_kwp_common.hpp): T = 303..306 and 607..610
    -- the last two sizes of one form and the first two of the next, among them the 2-wavefront form, which no other test
    launches, and T = 304 and 608, whose four and two wavefronts take exactly 80 KiB.  Wrap, and unwrap with every fifth
    record refused; n = 65 with headers and n = 64 waves + 1 (a second workgroup starts with one record) with NULL headers;
    src and dst 4-aligned (whole dwords at T = 304 and 608) and at 1 and 3 mod 4 (octets).  The plans are recomputed here, so
    that a retuned rule fails this test instead of leaving a form unlaunched"""
    plans = [G.plan(c + 16) for c in G.SEAM_COUNTS]
    assert {w for w, _ in plans} == {1, 2, 4} and {w for w, lds in plans if lds == 81920} == {2, 4}
    waves, lds = G.plan(count + 16)
    assert lds <= 80 * 1024
    eng = engine()
    j = G.SEAM_COUNTS.index(count)
    for n, hdrs in ((65, True), (64 * waves + 1, False)):
        b = G.batch(count, n, G.KEY_LENS[(j + n) % 3], seed=11, hdrs=hdrs, refuse=True)
        assert b.refused == list(range(2, n, 5)) and [i for i, c in enumerate(b.want_unwrap()[1]) if c] == b.refused
        for src_off, dst_off in ((0, 0), (1, 3)):
            check(eng, b, src_off=src_off, dst_off=dst_off)


def test_the_published_vector_inside_a_batch():
    """STB 34.101.31 A.21 as record 1 of 3 and A.22 as record 1 of 3"""
    eng, H = engine(), orclib.Golden().H
    a21 = bytes.fromhex("49A38EE108D6C742E52B774F00A6EF98B106CBD13EA4FB0680323051BC04DF76E487B055C69BCF541176169F1DC9F6C8")
    code, tokens = eng.beltKWP_wrap_batch(H[128:160], bytes(16) + H[32:48] + bytes(range(16)), bytes(32) + H[:32] + bytes(32), 32)
    assert code == 0 and tokens[48:96] == a21
    hdr22 = bytes.fromhex("B5EF68D8E4A39E567153DE13D72254EE")
    code, keys, codes = eng.beltKWP_unwrap_batch(H[160:192], bytes(16) + hdr22 + bytes(16), bytes(48) + H[64:112] + bytes(48), 48)
    assert code == 0 and codes == [E.ERR_BAD_KEYTOKEN, 0, E.ERR_BAD_KEYTOKEN]
    assert keys == bytes(32) + bytes.fromhex("92632EE0C21AD9E09A39343E5C07DAA4889B03F2E6847EB152EC99F7A4D9F154") + bytes(32)


# ================================================================================================ alignments
@pytest.mark.parametrize("count", [17, 24, 32])
def test_every_start_alignment_of_src_dst_and_headers(count):
    """each of the three bases at 0, 1, 2 and 3 mod 4 while the other two sit at two other residues, and all three 4-aligned
    (count 24 and 32: the dword rows); the codes start 4 mod 8 throughout"""
    eng = engine()
    b = G.batch(count, 65, 24, seed=5)
    offs = [(0, 0, 0)]
    for a in range(4):
        offs += [(a, 1, 2), (3, a, 1), (2, 3, a), (a, a, 4 + a)]
    for src_off, dst_off, hdr_off in offs:
        check(eng, b, src_off=src_off, dst_off=dst_off, hdr_off=hdr_off)


# ================================================================================================ refused tokens
@pytest.mark.parametrize("hdrs", [True, False], ids=["hdrs", "null-hdrs"])
@pytest.mark.parametrize("count", [16, 19, 24, 32])
def test_refused_tokens_are_zeroed_and_their_neighbours_stay(count, hdrs):
    """n = 257, every 5th record refused -- by a flipped token bit or by a header that differs in one bit from the one wrapped
    (with NULL headers: a token wrapped under a nonzero header): those records get ERR_BAD_KEYTOKEN and zeros, all others the
    key, and nothing else in the arena moved"""
    eng = engine()
    b = G.batch(count, 257, G.KEY_LENS[count % 3], seed=8, hdrs=hdrs, refuse=True)
    want, want_codes = b.want_unwrap()
    assert b.refused == list(range(2, 257, 5))
    assert [i for i, c in enumerate(want_codes) if c] == b.refused and {want_codes[i] for i in b.refused} == {E.ERR_BAD_KEYTOKEN}
    out, codes = run_unwrap(eng, b, b.tokens)
    assert codes == want_codes and out == want
    for i in range(257):
        assert out[count * i:count * (i + 1)] == (bytes(count) if i in b.refused else b.rec(i)), i


# ================================================================================================ the contract
def test_any_overlap_of_src_and_dst_is_refused_with_nothing_written():
    eng = engine()
    b = G.batch(32, 65)
    n_in, n_out = 65 * 32, 65 * 48
    A = Arena(7).add("buf", n_in + n_out + 64, 1).build()
    s, _ = A.at["buf"]
    codes = torch.zeros(65, dtype=torch.int32, device="cuda")
    for unwrap, count, src_len, dst_len in ((0, 32, n_in, n_out), (1, 48, n_out, n_in)):
        for src_at, dst_at in ((0, 0), (0, 1), (0, src_len - 1), (1, 0), (dst_len - 1, 0), (8, 0), (0, 8)):
            with pytest.raises(E.EngineError):
                eng.beltKWP_batch_stream(unwrap, b.key, None, A.dev[s + src_at:s + src_at + src_len], count, 65,
                                         A.dev[s + dst_at:s + dst_at + dst_len], codes)
    assert A.fetch([]) == {} and not codes.any()
    with pytest.raises(E.EngineError):                                # the codes 2 mod 4
        eng.beltKWP_batch_stream(1, b.key, None, A.dev[s:s + n_out], 48, 65, A.dev[s + n_out:s + n_out + n_in],
                                 A.dev[GUARD // 2 + 2:GUARD // 2 + 2 + 260])
    assert A.fetch([]) == {}


@pytest.mark.parametrize("unwrap", [0, 1], ids=["wrap", "unwrap"])
@pytest.mark.parametrize("count", [19, 32])
def test_side_stream_and_replay_from_a_graph_on_fresh_inputs(count, unwrap):
    """one eager call on a side stream, the same call captured on it (one queue: the entry forks nothing), replayed twice on
    refilled buffers, refused tokens among them"""
    eng = engine()
    b = G.batch(count, 129, 32, seed=6, refuse=True)
    outputs = ["dst", "codes"] if unwrap else ["dst"]

    def want(x):
        if not unwrap:
            return {"dst": x.tokens_clean}
        out, codes = x.want_unwrap()
        return {"dst": out, "codes": struct.pack(f"<{x.n}I", *codes)}

    A = arena(b, unwrap, b.tokens if unwrap else b.keys, seed=30)
    cap = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(cap):
        call(eng, b, A, unwrap)
    cap.synchronize()
    assert A.fetch(outputs) == want(b)
    A.refill()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cap):
        call(eng, b, A, unwrap)
    for seed in (41, 42):
        x = G.Batch(count, 129, 32, seed=seed, refuse=True, key=b.key)      # the key is baked into the captured launch
        A.put("src", x.tokens if unwrap else x.keys)
        A.put("hdrs", x.hdrs)
        A.refill()
        graph.replay()
        assert A.fetch(outputs) == want(x), seed


# ================================================================================================ host entries
@pytest.mark.parametrize("count", [16, 19, 24, 32, 240, 1008])
def test_host_entries_equal_the_model(count):
    """bee2hip_beltKWP_wrap_batch / _unwrap_batch on host pointers, refused tokens included, with and without headers"""
    eng = engine()
    for n, hdrs in ((65, True), (257, False)) if count < 1008 else ((65, True),):
        b = G.batch(count, n, G.KEY_LENS[count % 3], seed=8, hdrs=hdrs, refuse=True)
        assert eng.beltKWP_wrap_batch(b.key, b.hdrs, b.keys, count) == (E.ERR_OK, b.tokens_clean)
        want, want_codes = b.want_unwrap()
        assert eng.beltKWP_unwrap_batch(b.key, b.hdrs, b.tokens, b.T) == (E.ERR_OK, want, want_codes)


def test_host_entries_with_dst_equal_to_src():
    eng = engine()
    b = G.batch(33, 65, 24, seed=8, refuse=True)
    _sz = ctypes.c_size_t
    buf = ctypes.create_string_buffer(b.keys, 65 * b.T)
    assert eng.lib.bee2hip_beltKWP_wrap_batch(b.key, _sz(24), b.hdrs, buf, _sz(33), _sz(65), buf) == E.ERR_OK
    assert buf.raw == b.tokens_clean
    buf = ctypes.create_string_buffer(b.tokens, 65 * b.T)
    codes = (ctypes.c_uint32 * 65)()
    assert eng.lib.bee2hip_beltKWP_unwrap_batch(b.key, _sz(24), b.hdrs, buf, _sz(b.T), _sz(65), buf, codes) == E.ERR_OK
    want, want_codes = b.want_unwrap()
    assert buf.raw[:65 * 33] == want and list(codes) == want_codes and buf.raw[65 * 33:] == b.tokens[65 * 33:]


# ================================================================================================ inverse
@pytest.mark.parametrize("count", [16, 18, 31, 49, 240])
def test_unwrap_inverts_wrap_and_headers_separate_tokens(count):
    eng = engine()
    b = G.batch(count, 65, 32, seed=3)
    tokens = run_wrap(eng, b)
    assert tokens == b.tokens_clean
    out, codes = run_unwrap(eng, b, tokens, seed=4)
    assert out == b.keys and codes == [0] * 65
    same = G.Batch(count, 65, 32, seed=3)                             # equal keys under distinct headers: distinct tokens
    same.keys = same.keys[:count] * 65
    got = run_wrap(eng, same)
    assert len({got[same.T * i:same.T * (i + 1)] for i in range(65)}) == 65
    assert got == b"".join(M.wrap(same.rec(i), same.hdr(i), same.key) for i in range(65))
