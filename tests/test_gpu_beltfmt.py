"""-m gpu: the belt-fmt record batch (bee2hip_beltFMT_batch*, bee2_amd/csrc/belt_fmt_kernels.hip) and the drop-in beltFMTEncr /
beltFMTDecr against the plain-Python model, record by record, every output octet compared (tests/beltfmtgrid.py builds the
batches; tests/test_beltfmt.py pins the model to the reference).

The stream entry is a device-pointer batch entry that is not in the contract registry of tests/devcontract.py, so this file
holds it to the same contract itself, as tests/test_gpu_beltae.py does: every buffer is a slice of one allocation filled with a
seeded pattern, at the weakest alignment the header grants, with 4 KiB of pattern on each side; after a call the output is the
model's over its whole range and every other octet of the allocation -- inputs and guards -- is what it was."""
import random
import struct

import numpy as np
import pytest
import torch

import beltfmtgrid as G
import orc_beltfmt as M
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


def arena(b, src, inplace, src_off=2, dst_off=0, seed=1):
    """src at 256 k + src_off (2 mod 4 unless told otherwise), a separate dst at 256 k + dst_off, the ivs at an odd address"""
    A = Arena(seed).add("src", src, src_off)
    if not inplace:
        A.add("dst", len(src), dst_off)
    if b.ivs is not None:
        A.add("ivs", b.ivs, 5)
    return A.build()


def call(eng, b, A, decr):
    out = A.t("dst") if "dst" in A.at else A.t("src")
    eng.beltFMT_batch_stream(decr, b.mod, b.count, b.key, A.t("ivs") if "ivs" in A.at else None, A.t("src"), out, b.n)


def run(eng, b, decr, src, inplace, **kw):
    A = arena(b, src, inplace, **kw)
    call(eng, b, A, decr)
    name = "src" if inplace else "dst"
    return A.fetch([name])[name]


def check(eng, b):
    """both directions of batch b against the model, in place and into a separate dst"""
    for decr in (0, 1):
        want = b.want(decr)
        for inplace in (True, False):
            got = run(eng, b, decr, b.records, inplace, seed=2 + decr)
            assert got == want, (b.mod, b.count, b.n, decr, inplace, _first_bad(b, got, want))


def _first_bad(b, got, want):
    for i in range(b.n):
        lo, hi = 2 * b.count * i, 2 * b.count * (i + 1)
        if got[lo:hi] != want[lo:hi]:
            return i, struct.unpack(f"<{b.count}H", got[lo:hi]), struct.unpack(f"<{b.count}H", want[lo:hi])


# ================================================================================================ shapes
@pytest.mark.parametrize("shape", G.SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_shapes_at_every_batch_edge(shape):
    """b <= 4: one E_K, belt-32block, belt-wbl on 32 and on 40 octets, and the division by the moduli of the grid; n = 1, a
    partial, a whole and a started second wavefront, a started second workgroup.  Key lengths and iv / NULL iv rotate; every
    fifth record holds symbols at or above the modulus"""
    eng = engine()
    for j, n in enumerate((1, 63, 64, 65, 257)):
        check(eng, G.batch(shape[0], shape[1], n, G.KEY_LENS[j % 3], ivs=j != 3))


@pytest.mark.parametrize("shape", G.LARGE, ids=lambda s: f"{s[0]}x{s[1]}")
def test_large_shapes(shape):
    """56 and 64 octets of belt-wbl, the block-count exception on one half and on both, the maximum count at the smallest odd
    modulus, the largest numbers (b = 75: one wavefront per workgroup)"""
    check(engine(), G.batch(shape[0], shape[1], 65, G.KEY_LENS[G.LARGE.index(shape) % 3]))


@pytest.mark.parametrize("shape", G.PLAN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_both_sides_of_both_seams_of_the_launch_plan(shape):
    """the launcher picks 4, 2 or 1 wavefronts per workgroup from the LDS a wavefront needs (fmt_plan, belt_fmt_common.hpp):
    the last count of one form and the first of the next, at five moduli -- the 2-wavefront form, the 4- and 2-wavefront forms
    at exactly 80 KiB, the 1-wavefront form at its smallest.  n starts a second workgroup with one record (65 at the two
    moduli where the model is slow: a second wavefront).  Key lengths and iv / NULL iv rotate.  The plans are recomputed
    here, so that a retuned rule fails this test instead of leaving a form unlaunched"""
    plans = [G.plan(*s) for s in G.PLAN_SHAPES]
    assert {w for w, _ in plans} == {1, 2, 4} and any(lds == 81920 for _, lds in plans)
    assert {w for w, lds in plans if lds == 81920} == {2, 4}
    j = G.PLAN_SHAPES.index(shape)
    waves, lds = plans[j]
    n = G.plan_n(*shape)
    assert n in (65, 64 * waves + 1) and lds <= 80 * 1024
    check(engine(), G.batch(shape[0], shape[1], n, G.KEY_LENS[j % 3], ivs=j % 4 != 3))


@pytest.mark.parametrize("b", G.SWEEP_B)
def test_every_block_count_on_both_number_paths(b):
    """the trip counts of the kernel's Horner conversion, of its belt-wbl walk over 2 b + 2 limbs and of its shrinking division
    all come from b: every b = 1..40 with modulus 65536 (the number is the symbols) and 65535 (multiplication and division),
    at a count whose halves have b and b - 1 blocks, and b = 1..16 at modulus 10 (many divisions per limb); n = 65"""
    eng = engine()
    for j, (mod, count) in enumerate(G.SWEEP[b]):
        assert max(G.blocks(mod, count)) == b
        check(eng, G.batch(mod, count, 65, G.KEY_LENS[(b + j) % 3], ivs=(b + j) % 4 != 3))


@pytest.mark.parametrize("key_len", G.KEY_LENS)
@pytest.mark.parametrize("ivs", [True, False], ids=["ivs", "null-ivs"])
def test_every_key_length_with_and_without_ivs(key_len, ivs):
    eng = engine()
    for mod, count in ((10, 16), (58, 21), (65536, 17)):
        b = G.batch(mod, count, 65, key_len, seed=9, ivs=ivs)
        check(eng, b)
        if ivs:                                                     # distinct ivs give distinct results for equal records
            same = G.Batch(mod, count, 65, key_len, seed=9)
            same.rows = [same.rows[0]] * 65
            same.records = same.records[:2 * count] * 65
            got = run(eng, same, 0, same.records, True)
            assert len({got[2 * count * i:2 * count * (i + 1)] for i in range(65)}) == 65
            assert got == same.want(0)


@pytest.mark.parametrize("shape", [(10, 16), (10, 39), (257, 17), (36, 50), (65535, 32), (65536, 56), (3, 600)],
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_decryption_inverts_encryption(shape):
    eng = engine()
    b = G.batch(shape[0], shape[1], 65, 32, seed=3, oor=False)
    ct = run(eng, b, 0, b.records, True)
    assert ct != b.records and ct == b.want(0)
    assert run(eng, b, 1, ct, False, seed=4) == b.records
    syms = struct.unpack(f"<{65 * b.count}H", ct)
    assert max(syms) < b.mod                                         # the format is preserved


@pytest.mark.parametrize("shape", [(58, 21), (65536, 17), (257, 17), (10, 39)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_odd_counts_at_every_start_alignment(shape):
    """an odd count puts every second record at 2 mod 4 whatever the base is; the base itself at 0 and at 2 mod 4, the separate
    dst at the other residue"""
    eng = engine()
    b = G.batch(shape[0], shape[1], 65, 24, seed=5)
    for decr in (0, 1):
        for src_off, dst_off in ((0, 2), (2, 0), (2, 2), (6, 12)):
            assert run(eng, b, decr, b.records, False, src_off=src_off, dst_off=dst_off) == b.want(decr)
            assert run(eng, b, decr, b.records, True, src_off=src_off) == b.want(decr)


# ================================================================================================ the contract
def test_partial_overlap_is_refused_with_nothing_written():
    eng = engine()
    b = G.batch(10, 16, 65)
    A = Arena(7).add("buf", len(b.records) + 64, 2).build()
    s, n = A.at["buf"]
    for shift in (2, 30, 32, 64):
        for src, dst in ((A.dev[s:s + n - 64], A.dev[s + shift:s + shift + n - 64]), (A.dev[s + shift:s + shift + n - 64], A.dev[s:s + n - 64])):
            with pytest.raises(E.EngineError):
                eng.beltFMT_batch_stream(0, b.mod, b.count, b.key, None, src, dst, b.n)
    assert A.fetch([]) == {}
    with pytest.raises(E.EngineError):                                # 1 mod 2
        eng.beltFMT_batch_stream(0, b.mod, b.count, b.key, None, A.dev[s + 1:s + 1 + n - 64], A.dev[s + 1:s + 1 + n - 64], b.n)
    assert A.fetch([]) == {}


@pytest.mark.parametrize("decr", [0, 1], ids=["encr", "decr"])
@pytest.mark.parametrize("shape", [(10, 16), (65535, 32)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_side_stream_and_replay_from_a_graph_on_fresh_inputs(shape, decr):
    """one eager call on a side stream, the same call captured on it (one queue: the entry forks nothing), replayed twice on
    refilled buffers"""
    eng = engine()
    b = G.batch(shape[0], shape[1], 129, 32, seed=6)
    A = arena(b, b.records, False, seed=30)
    cap = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(cap):
        call(eng, b, A, decr)
    cap.synchronize()
    assert A.fetch(["dst"])["dst"] == b.want(decr)
    A.refill()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cap):
        call(eng, b, A, decr)
    for seed in (41, 42):
        x = G.Batch(b.mod, b.count, b.n, 32, seed=seed)
        x.key = b.key                                                # the key is baked into the captured launch
        A.put("src", x.records)
        A.put("ivs", x.ivs)
        A.refill()
        graph.replay()
        assert A.fetch(["dst"])["dst"] == x.want(decr), seed


# ================================================================================================ host entries
@pytest.mark.parametrize("shape", G.ALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_entry_equals_the_model(shape):
    """bee2hip_beltFMT_batch on host pointers, every shape, both directions: the 65-record batches of the shape tests above
    (without ivs for the small shapes, with them for the large ones), and (10, 16) once more with ivs"""
    eng = engine()
    if shape in G.SMALL:
        batches = [G.batch(shape[0], shape[1], 65, G.KEY_LENS[0], ivs=False)] + ([G.batch(10, 16, 64, G.KEY_LENS[2])] if shape == (10, 16) else [])
    else:
        batches = [G.batch(shape[0], shape[1], 65, G.KEY_LENS[G.LARGE.index(shape) % 3])]
    for b in batches:
        for decr in (0, 1):
            code, out = eng.beltFMT_batch(decr, b.mod, b.count, b.key, b.ivs, b.records)
            assert code == E.ERR_OK and out == b.want(decr), (b.n, decr)


def test_drop_in_one_shots_on_both_paths():
    """beltFMTEncr / beltFMTDecr: the standard's vectors and one record of every shape, by the kernel (policy 1) and by the host
    path (policy 2); bee2hip_path_count moves on the side it should; the policy is restored"""
    eng = engine()
    lib, H = eng.lib, orclib.Golden().H
    key, iv = H[128:160], H[192:208]
    try:
        for policy, side in ((1, 1), (2, 0)):
            lib.bee2hip_path_policy(policy)
            before = [lib.bee2hip_path_count(i) for i in range(3)]
            calls = 0
            for mod, vec in G.BEE2_VECTORS:
                src = list(range(len(vec)))
                assert eng.beltFMT(0, mod, src, key, iv) == (E.ERR_OK, vec)
                assert eng.beltFMT(1, mod, vec, key, iv) == (E.ERR_OK, src)
                calls += 2
            for mod, count in G.ALL_SHAPES:
                b = G.batch(mod, count, 65)
                i = 2 if policy == 1 else 3                            # record 2 holds symbols at or above the modulus
                for decr in (0, 1):
                    want = M.crypt(decr, mod, b.rows[i], b.key, b.iv(i))
                    assert eng.beltFMT(decr, mod, b.rows[i], b.key, b.iv(i)) == (E.ERR_OK, want), (policy, mod, count, decr)
                    calls += 1
            after = [lib.bee2hip_path_count(i) for i in range(3)]
            assert after[side] - before[side] == calls and after[1 - side] == before[1 - side] and after[2] == before[2]
    finally:
        lib.bee2hip_path_policy(0)
    # policy 0: a single record is one serial chain and runs on the host
    before = [lib.bee2hip_path_count(i) for i in range(3)]
    assert eng.beltFMT(0, 10, list(range(10)), key, iv) == (E.ERR_OK, G.BEE2_VECTORS[0][1])
    assert [lib.bee2hip_path_count(i) for i in range(3)] == [before[0] + 1, before[1], before[2]]
