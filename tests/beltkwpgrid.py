"""Counts, fixture rows and batches for belt-kwp (bee2_amd/csrc/belt_kwp_kernels.hip) and their expected outputs from the
plain-Python model (tests/orc_beltkwp.py, pinned to the reference by tests/golden/belt_kwp.json).  No GPU here:
tests/test_beltkwp.py runs the CPU side, tests/test_gpu_beltkwp.py the batches.  A `count` is always the WRAP count: the octets
of the wrapped key; the token has count + 16."""
import functools
import hashlib
import random

import orc_beltkwp as M

KEY_LENS = (16, 24, 32)
FIXTURE_COUNTS = list(range(16, 100)) + [127, 128, 129, 1007, 1008] + [288, 289, 592, 593]       # (append only: seeds come from the index)
# the shapes of the GPU batches: T = 32 (the sum is r1 alone); every tail residue mod 4; a dword tail that is not a multiple
# of 8; T = 40 (8 mod 16); around the A.21 shape; around four whole blocks; T = 256
GPU_COUNTS = [16, 17, 18, 19, 20, 24, 31, 32, 33, 47, 48, 49, 240]
GPU_COUNTS_CAP = [1007, 1008]                                      # one wavefront per workgroup
BATCH_SIZES = (1, 63, 64, 65, 257)
# both sides of the two changes of the launch plan: T = 303..306 (four wavefronts up to 304, then two) and 607..610 (two up to
# 608, then one); T = 304 and 608 are whole dwords, the others take the octet path
SEAM_COUNTS = [287, 288, 289, 290, 591, 592, 593, 594]


def plan(T):
    """kwp_plan() of belt_kwp_common.hpp restated -> (waves, lds); tests/test_beltkwp.py holds the two together"""
    wave_bytes = 256 * ((T + 3) // 4)
    waves = 4
    while waves > 1 and 4096 + waves * wave_bytes > 80 * 1024:
        waves //= 2
    return waves, 4096 + waves * wave_bytes


# ---- the committed fixture (tools/make_golden_beltkwp.py writes it from the reference): a row's inputs come from its seed
def fixture_cases():
    out = []
    for j, count in enumerate(FIXTURE_COUNTS):
        for k, key_len in enumerate(KEY_LENS):
            for header in (True, False):
                out.append({"count": count, "key_len": key_len, "header": header, "seed": 9000000 + 100 * j + 10 * k + header})
    return out


def case_inputs(c):
    """key, header (None: the NULL header), the octets to wrap, the token bit to flip (octet, bit) and a wrong header (a
    nonzero one for a row without header)"""
    rnd = random.Random(c["seed"])
    x = {"key": rnd.randbytes(c["key_len"]), "header": rnd.randbytes(16) if c["header"] else None, "src": rnd.randbytes(c["count"]),
         "flip": (rnd.randrange(c["count"] + 16), rnd.randrange(8))}
    wrong = bytearray(x["header"] or bytes(16))
    wrong[rnd.randrange(16)] ^= 1 << rnd.randrange(8)
    x["wrong_header"] = bytes(wrong)
    return x


def flipped(token, flip):
    t = bytearray(token)
    t[flip[0]] ^= 1 << flip[1]
    return bytes(t)


def encode(raw):
    """what the fixture records of an output: hex, or the sha256 above 64 octets"""
    return raw.hex() if len(raw) <= 64 else "sha256:" + hashlib.sha256(raw).hexdigest()


# ---- batches
class Batch:
    """n records of `count` octets under one key; hdrs: True = one header per record, False = NULL.  refuse: every 5th record
    (i % 5 == 2) of the UNWRAP input is spoilt -- by a flipped token bit, a flipped header bit (the header handed to unwrap
    differs from the one wrapped), in turn; with hdrs = False the second kind wraps under a nonzero header instead, so that
    the NULL header of the call meets a nonzero one"""

    def __init__(self, count, n, key_len=32, seed=0, hdrs=True, refuse=False, key=None):
        rnd = random.Random((count * 1000 + n) * 100 + key_len + 7919 * seed + (1 if hdrs else 0))
        self.count, self.n, self.T = count, n, count + 16
        self.key = rnd.randbytes(key_len)
        if key is not None:
            self.key = bytes(key)                                # (a captured launch keeps its key)
        self.hdrs = rnd.randbytes(16 * n) if hdrs else None
        self.keys = rnd.randbytes(count * n)                     # what is wrapped
        self.tokens_clean = b"".join(M.wrap(self.rec(i), self.hdr(i), self.key) for i in range(n))
        tokens, self.refused = bytearray(self.tokens_clean), []
        if refuse:
            for i in range(2, n, 5):
                kind = (i // 5) % 2
                lo = self.T * i
                if kind == 0:
                    tokens[lo + rnd.randrange(self.T)] ^= 1 << rnd.randrange(8)
                else:
                    wrong = bytearray(self.hdr(i) or bytes(16))
                    wrong[rnd.randrange(16)] ^= 1 << rnd.randrange(8)
                    tokens[lo:lo + self.T] = M.wrap(self.rec(i), bytes(wrong), self.key)
                self.refused.append(i)
        self.tokens = bytes(tokens)                               # the unwrap input
        self._want = None

    def rec(self, i):
        return self.keys[self.count * i:self.count * (i + 1)]

    def hdr(self, i):
        return None if self.hdrs is None else self.hdrs[16 * i:16 * i + 16]

    def want_unwrap(self):
        """(the output octets, [codes]) of unwrapping self.tokens, computed once"""
        if self._want is None:
            res = [M.unwrap(self.tokens[self.T * i:self.T * (i + 1)], self.hdr(i), self.key) for i in range(self.n)]
            self._want = (b"".join(r[1] for r in res), [r[0] for r in res])
        return self._want


@functools.lru_cache(maxsize=None)
def batch(count, n, key_len=32, seed=0, hdrs=True, refuse=False):
    return Batch(count, n, key_len, seed, hdrs, refuse)
