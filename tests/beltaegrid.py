"""Batches for the belt-dwp / belt-che record kernel (bee2_amd/csrc/belt_ae_kernels.hip) and their expected outputs, record
by record from the C oracle (orclib.dwp_wrap: oracle/oracle.h restates beltDWPWrap / beltCHEWrap and is pinned to the
reference by tests/golden/belt_ae_ragged.json, tests/test_beltae.py).  No GPU here: tests/test_beltae.py proves the coverage
on the CPU, tests/test_gpu_beltae.py runs the batches.

The (start mod 16) x length construction is that of tests/raggedgrid.py: before each wanted record goes a filler record of
0..15 octets that moves the cursor to the wanted residue.  The headers are packed the same way, so the filler's header is what
moves the wanted header to ITS residue; fillers are ordinary records of the batch and are checked like any other."""
import functools
import hashlib
import random

import orclib
from raggedgrid import build

MODES = {0: "DWP", 1: "CHE"}
KEY_LENS = (16, 24, 32)
# every residue mod 16 three times over, one to three blocks, the 8-block line
TEXT_LENS = list(range(0, 50)) + [63, 64, 65, 127, 128, 129, 255, 256, 257]
HDR_LENS = (0, 1, 15, 16, 17, 33)
HDR_RES = (0, 1, 7, 15)
ERR_OK, ERR_BAD_MAC = 0, 511


class Batch:
    def __init__(self, mode, key, blob, offsets, hdr_lens, seed, ivs=None):
        rnd = random.Random(seed ^ 0xBE17)
        self.mode, self.key = mode, bytes(key)
        self.blob, self.offsets = bytes(blob), list(offsets)
        self.n = n = len(offsets) - 1
        self.ivs = rnd.randbytes(16 * n) if ivs is None else bytes(ivs)
        self.hoffsets = [0]
        for h in hdr_lens:
            self.hoffsets.append(self.hoffsets[-1] + h)
        self.hblob = rnd.randbytes(self.hoffsets[-1])
        self._want = None

    def text(self, i, blob=None):
        return (self.blob if blob is None else blob)[self.offsets[i]:self.offsets[i + 1]]

    def hdr(self, i, hblob=None):
        return (self.hblob if hblob is None else hblob)[self.hoffsets[i]:self.hoffsets[i + 1]]

    def iv(self, i, ivs=None):
        return (self.ivs if ivs is None else ivs)[16 * i:16 * i + 16]

    def want(self):
        """(ciphertext blob, tags) of the whole batch from the oracle, computed once"""
        if self._want is None:
            orc = orclib.load()
            ct, tags = bytearray(), bytearray()
            for i in range(self.n):
                code, c, t = orc.dwp_wrap(self.text(i), self.hdr(i), self.key, self.iv(i), MODES[self.mode])
                assert code == 0
                ct += c
                tags += t
            self._want = (bytes(self.blob[:self.offsets[0]]) + bytes(ct), bytes(tags))
        return self._want

    def order(self):
        """longest text first, as the host entries sort"""
        return sorted(range(self.n), key=lambda i: self.offsets[i] - self.offsets[i + 1])


def grid_header_lens(n):
    """header lengths of the n = 2 k records of a grid batch (filler, wanted, filler, wanted ..): wanted record number w has
    HDR_LENS[w % 6] octets starting at HDR_RES[(w // 6) % 4] mod 16, the filler before it whatever moves the cursor there"""
    lens, cursor = [], 0
    for w in range(n // 2):
        f = (HDR_RES[(w // 6) % 4] - cursor) % 16
        h = HDR_LENS[w % 6]
        lens += [f, h]
        cursor += f + h
    return lens


def header_coverage(b):
    """the set of (start mod 16, length) over the headers of the wanted (odd) records"""
    return {(b.hoffsets[i] % 16, b.hoffsets[i + 1] - b.hoffsets[i]) for i in range(1, b.n, 2)}


@functools.lru_cache(maxsize=None)
def grid(mode, key_len=32):
    seed = 3100 + 10 * mode + key_len
    blob, offsets = build(TEXT_LENS, seed)
    n = len(offsets) - 1
    return Batch(mode, random.Random(seed ^ 0x4B).randbytes(key_len), blob, offsets, grid_header_lens(n), seed)


def pack(lens, seed):
    offsets = [0]
    for x in lens:
        offsets.append(offsets[-1] + x)
    return random.Random(seed).randbytes(offsets[-1]), offsets


LONG = (4095, 4096, 4097, 6000)


@functools.lru_cache(maxsize=None)
def edge(n, mode, key_len=32):
    """n records: short ones of 0 .. 300 octets with empty records among them and, once there is room, four long ones placed
    apart; headers of 0 .. 40 octets"""
    seed = 91 * n + mode + key_len
    rnd = random.Random(seed)
    lens = [0 if rnd.random() < 0.1 else rnd.randrange(0, 301) for _ in range(n)]
    if n >= 63:
        for k, L in enumerate(LONG):
            lens[(k * n) // len(LONG) + 3] = L
    blob, offsets = pack(lens, seed + 1)
    hl = [rnd.choice((0, 0, 1, 7, 15, 16, 17, 40)) for _ in range(n)]
    return Batch(mode, rnd.randbytes(key_len), blob, offsets, hl, seed)


# ---- the committed fixture (tools/make_golden_beltae.py writes it from the reference): a record's inputs come from its seed
def case_inputs(c):
    rnd = random.Random(c["seed"])
    return {"key": rnd.randbytes(c["key_len"]), "iv": rnd.randbytes(16), "hdr": rnd.randbytes(c["hdr_len"]),
            "text": rnd.randbytes(c["text_len"])}


def fixture_cases():
    """both modes x the three key lengths x every text length of the grid; the header lengths cycle"""
    out = []
    for mode in (0, 1):
        for k, key_len in enumerate(KEY_LENS):
            for j, text_len in enumerate(TEXT_LENS):
                out.append({"mode": mode, "key_len": key_len, "text_len": text_len, "hdr_len": HDR_LENS[(j + k) % 6],
                            "seed": 100000 * mode + 1000 * key_len + j})
    return out


# the carry record: belt-dwp under CARRY_KEY with the committed iv of the fixture, whose counter s = E_K(iv) has
# s mod 2^32 >= 2^32 - 2^12, so that s + j carries out of the low word for some block j <= 2^12 of its 2^12 + 16 blocks
CARRY_KEY = bytes(range(0x40, 0x60))
CARRY_BLOCKS = (1 << 12) + 16
CARRY_SEED = 0xCA11


def carry_inputs(iv_hex):
    rnd = random.Random(CARRY_SEED)
    return {"key": CARRY_KEY, "iv": bytes.fromhex(iv_hex), "hdr": rnd.randbytes(21), "text": rnd.randbytes(16 * CARRY_BLOCKS)}


def carry_counter(orc, iv):
    """s mod 2^32 of the record: the low word of E_K(iv)"""
    code, s = orc.ecb(iv, CARRY_KEY)
    assert code == 0
    return int.from_bytes(s[:4], "little")


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()
