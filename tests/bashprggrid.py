"""Batches for the bash-prg kernel (bee2_amd/csrc/bash_prg_kernels.hip) and their expected outputs from the Python model
(tests/orc_bashprg.py).  No GPU here: tests/test_bashprg.py proves the coverage on the CPU, tests/test_gpu_bashprg.py runs the
batches.  The (start mod 16) x length construction is that of tests/raggedgrid.py; what is added per record is a header (its
lengths cycle through 0, 1, r-1, r, r+1) and an announcement, per batch a key, an announcement length and a tag length."""
import functools
import random

import orc_bashprg as M
from raggedgrid import build

ANN_LENS = (0, 4, 16, 60)
TAG_LENS = (1, 8, 32, 64)


def grid_lengths(r):
    """0 .. r+17 (every tail length and the first block boundary, across a quad), around two blocks, 3r-16 .. 3r+1"""
    return list(range(0, r + 18)) + [2 * r - 1, 2 * r, 2 * r + 1] + list(range(3 * r - 16, 3 * r + 2))


def key_lens(l):
    return list(range(l // 8, 61, 4))


def grid_config(l, c):
    """configuration c = 0..3 of a grid run: (ann_len, key_len, tag_len); the key lengths step from l/8 to 60"""
    ks = key_lens(l)
    return ANN_LENS[c], ks[c * (len(ks) - 1) // 3], TAG_LENS[c]


def header_lens(r, n):
    cyc = (0, 1, r - 1, r, r + 1)
    return [cyc[i % 5] for i in range(n)]


class AEBatch:
    def __init__(self, l, d, key, ann_len, tag_len, blob, offsets, hdr_lens, seed):
        rnd = random.Random(seed ^ 0xAE)
        self.l, self.d, self.key, self.ann_len, self.tag_len = l, d, bytes(key), ann_len, tag_len
        self.blob, self.offsets = bytes(blob), list(offsets)
        self.n = n = len(offsets) - 1
        self.anns = rnd.randbytes(n * ann_len)
        self.hoffsets = [0]
        for h in hdr_lens:
            self.hoffsets.append(self.hoffsets[-1] + h)
        self.hblob = rnd.randbytes(self.hoffsets[-1])
        self._want = None

    def text(self, i, blob=None):
        return (self.blob if blob is None else blob)[self.offsets[i]:self.offsets[i + 1]]

    def hdr(self, i, hblob=None):
        return (self.hblob if hblob is None else hblob)[self.hoffsets[i]:self.hoffsets[i + 1]]

    def ann(self, i, anns=None):
        return (self.anns if anns is None else anns)[i * self.ann_len:(i + 1) * self.ann_len]

    def want(self):
        """(ciphertext blob, tags) of the whole batch from the model, computed once"""
        if self._want is None:
            ct, tags = bytearray(), bytearray()
            for i in range(self.n):
                c, t = M.ae_wrap(self.l, self.d, self.key, self.ann(i), self.hdr(i), self.text(i), self.tag_len)
                ct += c
                tags += t
            self._want = (bytes(self.blob[:self.offsets[0]]) + bytes(ct), bytes(tags))
        return self._want

    def order(self):
        """longest text first, as the host entries sort"""
        return sorted(range(self.n), key=lambda i: self.offsets[i] - self.offsets[i + 1])


@functools.lru_cache(maxsize=None)
def ae_grid(l, d, c):
    """the length x alignment grid of (l, d) in configuration c"""
    r = M.rate(l, d, True)
    ann_len, key_len, tag_len = grid_config(l, c)
    seed = 1000 * l + 10 * d + c
    blob, offsets = build(grid_lengths(r), seed)
    key = random.Random(seed ^ 0x4B).randbytes(key_len)
    return AEBatch(l, d, key, ann_len, tag_len, blob, offsets, header_lens(r, len(offsets) - 1), seed)


class HashBatch:
    def __init__(self, l, d, ann, out_len, blob, offsets):
        self.l, self.d, self.ann, self.out_len = l, d, bytes(ann), out_len
        self.blob, self.offsets, self.n = bytes(blob), list(offsets), len(offsets) - 1
        self._want = None

    def msg(self, i):
        return self.blob[self.offsets[i]:self.offsets[i + 1]]

    def want(self):
        if self._want is None:
            self._want = b"".join(M.prg_hash(self.l, self.d, self.ann, self.msg(i), self.out_len) for i in range(self.n))
        return self._want

    def order(self):
        return sorted(range(self.n), key=lambda i: self.offsets[i] - self.offsets[i + 1])


@functools.lru_cache(maxsize=None)
def hash_grid(l, d, c):
    r = M.rate(l, d, False)
    seed = 2000 * l + 10 * d + c
    blob, offsets = build(grid_lengths(r), seed)
    return HashBatch(l, d, random.Random(seed ^ 0xA).randbytes(ANN_LENS[c]), TAG_LENS[c], blob, offsets)


LONG = (4095, 4096, 4097, 20000)


def edge_lengths(n, r, seed):
    """n record lengths: short ones of 0 .. 2r+40 octets with empty records among them and, once there is room, the long
    records placed apart"""
    rnd = random.Random(seed)
    lens = [0 if rnd.random() < 0.1 else rnd.randrange(0, 2 * r + 41) for _ in range(n)]
    if n >= 63:
        for k, L in enumerate(LONG):
            lens[(k * n) // len(LONG) + 3] = L
    return lens


def pack(lens, seed):
    offsets = [0]
    for x in lens:
        offsets.append(offsets[-1] + x)
    return random.Random(seed).randbytes(offsets[-1]), offsets


@functools.lru_cache(maxsize=None)
def ae_edge(n, l, d):
    r = M.rate(l, d, True)
    seed = 77 * n + l + d
    rnd = random.Random(seed)
    blob, offsets = pack(edge_lengths(n, r, seed), seed + 1)
    hl = [rnd.choice((0, 0, 1, 7, r - 1, r, r + 1, 2 * r + 3)) for _ in range(n)]
    return AEBatch(l, d, rnd.randbytes(rnd.choice(key_lens(l))), rnd.choice(ANN_LENS), rnd.choice(TAG_LENS), blob, offsets, hl, seed)


@functools.lru_cache(maxsize=None)
def hash_edge(n, l, d):
    r = M.rate(l, d, False)
    seed = 79 * n + l + d
    rnd = random.Random(seed)
    blob, offsets = pack(edge_lengths(n, r, seed), seed + 1)
    return HashBatch(l, d, rnd.randbytes(rnd.choice(ANN_LENS)), rnd.choice(TAG_LENS), blob, offsets)
