"""-m gpu: the edges of bashF_tile_kernel's tile (bee2_amd/csrc/bashf_tile.hpp).  A full tile of 64 states takes the fast path
(no clamp, no per-piece bounds, pipelined half-slab passes), any other tile the general path; the batch sizes put a lone partial
tile on each side of the half-slab boundary (1, 31, 32, 33, 63), exactly one fast-path tile (64), a fast-path tile beside a partial
one in the same workgroup (65, 128, 255), a full workgroup plus one state (257) and partial tiles behind several full ones."""
import functools

import pytest
import torch

from gpulib import dev, engine, host

pytestmark = pytest.mark.gpu

SIZES = [1, 31, 32, 33, 63, 64, 65, 128, 255, 256, 257, 64 * 5 + 32, 64 * 5 + 33, 64 * 7 + 63, 64 * 8]
GUARD = bytes((37 * i + 11) & 0xFF for i in range(4096))


@functools.lru_cache(maxsize=None)
def _states():
    """max(SIZES) seeded states and their images, computed once: the states are independent, so a batch of n is a prefix"""
    import orclib
    orc = orclib.load()
    data = orc.fill(192 * max(SIZES), 0xED6E)
    return data, orc.bashF_batch(data)


@pytest.mark.parametrize("n", SIZES)
def test_bashF_batch_dev_against_the_oracle(n):
    data, want = _states()
    t = dev(data[: 192 * n])
    engine().bashF_batch_dev(t)
    torch.cuda.synchronize()
    assert host(t) == want[: 192 * n]


@pytest.mark.parametrize("n", SIZES)
def test_bashF_batch_dev_leaves_a_4KiB_guard_untouched(n):
    """the fast path has no bounds of its own: a partial launch must never reach it with a short tile"""
    data, want = _states()
    t = dev(data[: 192 * n] + GUARD)
    engine().bashF_batch_dev(t[: 192 * n])
    torch.cuda.synchronize()
    out = host(t)
    assert out[192 * n:] == GUARD
    assert out[: 192 * n] == want[: 192 * n]


def test_golden_batch_with_A2_in_slot0(golden):
    t = dev(golden.bashf_in)
    engine().bashF_batch_dev(t)
    torch.cuda.synchronize()
    out = host(t)
    assert out[:192].hex() == golden.kat["bashF_A2"]["out"]
    assert out == golden.bashf_out
