"""-m gpu: the ragged hash kernels behind launch_hash_ragged (bee2_amd/csrc/mixed_kernels.hip) on the batches of tests/raggedgrid.py:
every length of a set at all 16 start alignments, in every form the dispatch picks by batch size and message length.  Digests
byte for byte against the oracle (orc.belt_hash, orc.bashHash); the digest array is pattern-filled and one guard slot behind it
must survive; data tensors carry 16 octets of slack, as a caller's do.  tests/test_ragged_grid.py proves on the CPU that the
batches hold every (alignment, length) pair."""
import random

import numpy as np
import pytest
import torch

import raggedgrid as RG
from gpulib import dev, engine

pytestmark = pytest.mark.gpu

FILL = 0xA5


class Batch:
    """a batch on the device with its expected digests (one oracle call per distinct message, computed once per batch)"""

    def __init__(self, orc, alg, blob, offsets):
        self.alg, self.dl, self.n = alg, RG.DIGEST[alg], len(offsets) - 1
        self.blob = blob
        self.off = np.asarray(offsets, dtype=np.int64)
        self.lens = np.diff(self.off)
        one = (lambda m: orc.belt_hash(m)) if alg == 0 else (lambda m: orc.bashHash(alg, m)[1])
        want = np.empty((self.n, self.dl), dtype=np.uint8)
        empty = np.frombuffer(one(b""), dtype=np.uint8)
        want[self.lens == 0] = empty                                     # (the padding of the large batches: in bulk)
        seen = {}
        for i in np.flatnonzero(self.lens):
            m = blob[self.off[i]:self.off[i + 1]]
            d = seen.get(m)
            if d is None:
                d = seen[m] = np.frombuffer(one(m), dtype=np.uint8)
            want[i] = d
        self.want = want
        self.data = dev(blob + bytes(16))
        self.doff = torch.from_numpy(self.off).cuda()

    def run(self, eng, order=None, first=0, count=None):
        """one launch over messages first .. first + count; -> the digests as an (count, dl) array"""
        count = self.n - first if count is None else count
        dig = torch.full(((count + 1) * self.dl,), FILL, dtype=torch.uint8, device="cuda")
        o = None if order is None else torch.from_numpy(np.asarray(order, dtype=np.int32)).cuda()
        eng.hash_ragged_dev(self.alg, self.data, self.doff[first:], dig, count, order=o)
        eng.sync()
        got = dig.cpu().numpy().reshape(count + 1, self.dl)
        assert (got[count] == FILL).all(), "the guard slot behind the digests was written"
        return got[:count]

    def check(self, got, what, first=0):
        want = self.want[first: first + len(got)]
        bad = np.flatnonzero((got != want).any(axis=1))
        # (alg, case, how many, then index / start mod 16 / length of the first few: what a kernel fix starts from)
        assert bad.size == 0, (self.alg, what, int(bad.size),
                               [(int(first + i), int(self.off[first + i] % 16), int(self.lens[first + i])) for i in bad[:8]])


@pytest.mark.parametrize("alg", RG.ALGS)
def test_short_forms_every_length_at_every_start_alignment(orc, alg):
    """belt_hash_ragged_kernel<BeltTabSmall, 64> (alg 0) and bash_ragged_kernel<16> / <12> / <8> (bash256 / 384 / 512): lengths
    0 .. B+17, 2B-1 .. 2B+1 and 3B-16 .. 3B+1 (B = 32 / 128 / 96 / 64 octets) at all 16 values of p mod 16 -- the two mask selects
    and the alignbit shift against every tail length of the keep / pad masks, whose loop extents (NQ, W / A / B) follow the rate.
    Three ways in: the library's device bucketing (ragged_hist / _scan / _scatter, n >= 128; from 1024 messages the short kernel
    runs on the side stream), a caller's random order, and launches of 127 messages (no order at all)."""
    eng = engine()
    lengths = RG.short_lengths(alg)
    blob, off = RG.build(lengths, 0x5407 + alg)
    assert RG.missing(off, lengths) == []
    b = Batch(orc, alg, blob, off)
    b.check(b.run(eng), "bucketed")
    perm = random.Random(alg + 1).sample(range(b.n), b.n)
    b.check(b.run(eng, order=perm), "ordered")
    for lo, cnt in RG.chunks(b.n, 127):
        b.check(b.run(eng, first=lo, count=cnt), f"unordered {lo}..{lo + cnt}", first=lo)


@pytest.mark.parametrize("alg", RG.ALGS)
def test_long_forms_every_start_alignment_and_tail(orc, alg):
    """belt_hash_long_kernel<BeltTabSmall, 64, 8> (alg 0: sh = (p & 3) * 8, the nine-word prefetch W[8] / Wn[8], the zero-padded last
    block by len mod 32) and bash_long_kernel<16> / <12> / <8> (load64_any at every p mod 8, the tail `pos < left ? .. : pos == left
    ? 0x40 : 0` by len mod RATE, row 1 inside / outside the rate): 4096, 4097, 4096 + 31 / 32 / 33, 4096 + B - 1 / B / B + 1, 8191,
    8192, 8193 at all 16 start alignments; 4095 beside them is the last length the short kernel owns (`len >= long_from`)."""
    eng = engine()
    lengths = RG.long_lengths(alg)
    blob, off = RG.build(lengths, 0x1076 + alg)
    assert RG.missing(off, lengths) == []
    b = Batch(orc, alg, blob, off)
    b.check(b.run(eng), "bucketed")
    perm = random.Random(alg + 2).sample(range(b.n), b.n)
    b.check(b.run(eng, order=perm), "ordered")


def _regime_n(kind):
    if kind == "wide":
        n = torch.cuda.get_device_properties(0).multi_processor_count * 1024 + 5
        if n > 1 << 19:
            pytest.skip(f"{n} messages: more than 2^19")
        return n
    return kind


_regime_cache = {}


def _regime(orc, alg, n):
    """(built once per (alg, n): the device and the host-pointer case share the 2^16 + 3 belt-hash batch)"""
    if (alg, n) not in _regime_cache:
        _regime_cache.clear()
        blob, off = RG.regime_batch(alg, n, n)
        assert RG.missing(off, RG.long_lengths(alg)) == []
        _regime_cache[(alg, n)] = Batch(orc, alg, blob, off)
    return _regime_cache[(alg, n)]


@pytest.mark.parametrize("alg,kind", [(0, 32767), (0, 1 << 16), (0, "wide"), (128, (1 << 16) + 3), (256, (1 << 16) + 3), (0, (1 << 16) + 3)],
                         ids=lambda v: str(v))
def test_long_grid_in_each_size_regime(orc, alg, kind):
    """The long grid (every long length at all 16 alignments) inside batches of each size at which launch_hash_ragged changes
    kernels, 2000 messages of 1..199 octets and empty messages filling up to n:
      n = 32767        belt_hash_long_kernel<.., 8> beside belt_hash_ragged_kernel<BeltTabSmall, 64>
      n = 2^16         belt_hash_long_kernel<.., 8> (its last size) beside belt_hash_ragged_kernel<BeltTabTwoP, 256>
      n = 2^16 + 3     belt_hash_long_kernel<BeltTabSmall, 64, 2>, the PAIR form (slot = lane / 2, `odd` from lane bit 0, its prefetch
                       and its zero-padded tail produce digests here), beside belt_hash_ragged_kernel<BeltTabTwoP, 256> and its
                       `len >= long_from` exit; bash_long_kernel<16> / <8> on an n * 8 grid beside bash_ragged_kernel (alg 128, 256)
      n = CUs * 1024 + 5   the pair form beside belt_hash_ragged_kernel<BeltTabTwoP, 1024>
    each once with the library's bucketing (ragged_hist / _scan / _scatter with populated buckets of 2^12 and 2^13 and n > 2^16: the
    chains in the first slots) and once in a caller's random order (the chains anywhere in the grid), both on the forked side stream."""
    eng = engine()
    n = _regime_n(kind)
    b = _regime(orc, alg, n)
    assert b.n == n
    b.check(b.run(eng), "bucketed")
    perm = np.random.default_rng(n).permutation(n)
    b.check(b.run(eng, order=perm), "ordered")


def test_host_pointer_entry_on_the_pair_form_batch(orc):
    """bee2hip_hash_ragged (host pointers) on the 2^16 + 3 belt-hash batch: its own longest-first order, the upload, then
    belt_hash_long_kernel<BeltTabSmall, 64, 2> and belt_hash_ragged_kernel<BeltTabTwoP, 256> through the ordered device entry.  No
    message reaches 64 KiB, so none goes to host threads: bee2hip_path_count(0) does not move."""
    eng = engine()
    n = (1 << 16) + 3
    b = _regime(orc, 0, n)
    msgs = [b.blob[b.off[i]:b.off[i + 1]] for i in range(n)]
    before = eng.lib.bee2hip_path_count(0)
    code, digs = eng.hash_ragged(0, msgs)
    assert code == 0 and eng.lib.bee2hip_path_count(0) == before
    got = np.frombuffer(b"".join(digs), dtype=np.uint8).reshape(n, 32)
    b.check(got, "host pointers")
