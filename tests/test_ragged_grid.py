"""CPU tests: the batches of tests/raggedgrid.py hold what the GPU tests rely on -- every (start mod 16, length) pair of every
length set, and all 16 start alignments among the items of the signing cases.  A builder (or a length set) that silently drops
a class fails here, without a GPU."""
import pytest

import raggedgrid as RG


def test_length_sets_are_the_ones_the_kernels_need():
    for alg in RG.ALGS:
        B = RG.BLOCK[alg]
        s = RG.short_lengths(alg)
        assert len(set(s)) == len(s) and max(s) < RG.LONG_FROM
        assert set(range(0, B + 18)) <= set(s) and {2 * B - 1, 2 * B, 2 * B + 1} <= set(s) and set(range(3 * B - 16, 3 * B + 2)) <= set(s)
        assert {L % B for L in s} == set(range(B))                     # every tail length of the keep / pad masks
        g = RG.long_lengths(alg)
        assert {4095, 4096, 4097, 4096 + 31, 4096 + 32, 4096 + 33, 4096 + B - 1, 4096 + B, 4096 + B + 1, 8191, 8192, 8193} == set(g)
        assert [L for L in g if L < RG.LONG_FROM] == [4095]


@pytest.mark.parametrize("alg", RG.ALGS)
def test_short_grid_has_every_alignment_of_every_length(alg):
    lengths = RG.short_lengths(alg)
    blob, off = RG.build(lengths, 0x5407 + alg)
    assert RG.missing(off, lengths) == []
    n = len(off) - 1
    assert n == 2 * 16 * len(lengths) and n >= 1024                    # (bucketed on the device, short kernel on the side stream)
    assert len(blob) == off[-1] and all(off[i] <= off[i + 1] for i in range(n))
    assert all(off[i + 1] - off[i] < 16 for i in range(0, n, 2))       # the fillers
    # cut into launches of fewer than 128 messages (no bucketing) nothing is lost
    cut = RG.chunks(n, 127)
    assert all(c < 128 for _, c in cut) and sum(c for _, c in cut) == n and [lo for lo, _ in cut] == list(range(0, n, 127))


@pytest.mark.parametrize("alg", RG.ALGS)
def test_long_grid_has_every_alignment_of_every_length(alg):
    lengths = RG.long_lengths(alg)
    blob, off = RG.build(lengths, 0x1076 + alg)
    assert RG.missing(off, lengths) == []
    assert 128 <= len(off) - 1 < 1024 and len(blob) == off[-1] < 3 << 20


@pytest.mark.parametrize("alg,n", [(0, 32767), (0, 1 << 16), (0, (1 << 16) + 3), (0, 256 * 1024 + 5), (0, 304 * 1024 + 5),
                                   (128, (1 << 16) + 3), (256, (1 << 16) + 3)])
def test_size_regime_batches_keep_the_long_grid(alg, n):
    blob, off = RG.regime_batch(alg, n, n)
    assert len(off) == n + 1 and len(blob) == off[-1]
    assert RG.missing(off, RG.long_lengths(alg)) == []
    lens = [off[i + 1] - off[i] for i in range(n)]
    assert sum(1 for L in lens if 16 <= L < 200) > RG.REGIME_SHORT * 0.85        # the short kernel has work beside the chains
    assert sum(1 for L in lens if L >= RG.LONG_FROM) == 16 * (len(RG.long_lengths(alg)) - 1)
    assert lens.count(0) >= n - 2 * 16 * len(RG.long_lengths(alg)) - RG.REGIME_SHORT
    assert max(lens) < 65536                                                      # nothing the host-pointer entry would offload


def test_builder_reports_a_dropped_class():
    """the check itself: a batch without its fillers, or with one message removed, is reported"""
    lengths = [6, 34]
    blob, off = RG.build(lengths, 1)
    assert RG.missing(off, lengths) == []
    packed = [0]
    for L in lengths:
        for _ in range(16):
            packed.append(packed[-1] + L)
    assert len(RG.missing(packed, lengths)) == 16            # back to back, even lengths only ever start at even offsets
    assert RG.missing(off[:-1], lengths) == [(15, 34)]       # the last message cut off


@pytest.mark.parametrize("l", [128, 192, 256])
def test_signing_items_start_at_all_16_alignments(l):
    """bee2hip_bignSign2_batch with t_len > 64 lays item i at i * ml, ml = oid_len + l/4 + t_len: with ml odd the 67 items reach all
    16 alignments (the case the GPU test relies on), and the even ml of the list are known not to"""
    from bee2_amd.engine import LEVEL_OID
    assert len(LEVEL_OID[l]) == RG.SIGN_OID_LEN
    t_odd = RG.SIGN_T_ODD[l]
    assert t_odd > 64 and RG.sign_ml(l, t_odd) % 2 == 1
    assert RG.sign_alignments(l, t_odd) == set(range(16))
    for t_len in RG.SIGN_T_SHARED:
        if t_len > 64 and RG.sign_ml(l, t_len) % 2 == 1:
            assert RG.sign_alignments(l, t_len) == set(range(16))
    # the list holds both sides of the 64-octet boundary and a message the kernel walks through 4 KiB and more
    assert {63, 64, 65} <= set(RG.SIGN_T_SHARED) and max(RG.sign_ml(l, t) for t in RG.SIGN_T_SHARED) >= 4096 + 32
    assert set(RG.SIGN_T_DEV) == {1, 31, 32, 33, 63, 64}
