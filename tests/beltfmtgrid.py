"""Shapes, fixture rows and batches for belt-fmt (bee2_amd/csrc/belt_fmt_kernels.hip, host_fmt.hpp) and their expected outputs
from the plain-Python model (tests/orc_beltfmt.py, pinned to the reference by tests/golden/belt_fmt.json).  No GPU here:
tests/test_beltfmt.py runs the CPU side, tests/test_gpu_beltfmt.py the batches."""
import functools
import hashlib
import random
import struct

import orc_beltfmt as M

KEY_LENS = (16, 24, 32)
# (mod, count): each the smallest member of its class -- see the b1 / b2 column of the fixture
SHAPES = [(2, 2), (10, 16), (256, 16), (10, 39), (58, 21), (257, 17), (65536, 17), (36, 50), (65536, 32), (65535, 32),
          (65536, 48), (65536, 56), (49667, 319), (49667, 320), (3, 600), (65521, 599), (65536, 600)]
DIV_MODS = (2, 3, 255, 257, 32768, 32769, 65521, 65535)          # the division by a run-time modulus, at count 16
DIV_SHAPES = [(m, 16) for m in DIV_MODS]
ALL_SHAPES = SHAPES + [s for s in DIV_SHAPES if s not in SHAPES]


def blocks(mod, count):
    return M.block_count(mod, (count + 1) // 2), M.block_count(mod, count // 2)


SMALL = [s for s in ALL_SHAPES if max(blocks(*s)) <= 4]
LARGE = [s for s in ALL_SHAPES if max(blocks(*s)) > 4]


# ---- the launch plan: fmt_plan() of belt_fmt_common.hpp restated (tests/test_beltfmt.py holds the two together)
TAB_BYTES, WG_LDS_MAX = 4096, 80 * 1024


def plan(mod, count):
    """-> (waves, lds): a wavefront owns 256 (2 max(b1, b2) + 2) octets of numbers and 128 count of records; 4, 2 or 1
    wavefronts per workgroup, as many as keep the workgroup within 80 KiB"""
    wave_bytes = 256 * (2 * max(blocks(mod, count)) + 2) + 128 * count
    waves = 4
    while waves > 1 and TAB_BYTES + waves * wave_bytes > WG_LDS_MAX:
        waves //= 2
    return waves, TAB_BYTES + waves * wave_bytes


# mod: (the last count with 4 wavefronts, the last count with 2): the plan changes form behind each
SEAMS = {2: (140, 288), 10: (132, 268), 58: (124, 252), 257: (116, 238), 65535: (96, 200), 65536: (96, 200)}
# both sides of both seams; at (2, 140), (10, 132), (257, 116) four wavefronts take exactly 80 KiB, at (2, 288), (65535, 200)
# and (65536, 200) two do
PLAN_SHAPES = [(mod, c + d) for mod in (2, 10, 257, 65535, 65536) for c in SEAMS[mod] for d in (0, 1)]


def plan_n(mod, count):
    """the batch size of a seam shape: a second workgroup starts with one record; one started second wavefront where the
    model is slow (the small moduli: many symbols per number)"""
    return 65 if mod in (2, 257) else 64 * plan(mod, count)[0] + 1


# ---- every block count 1..40, on the 2^16 path (65536) and on the division path (65535): at count 8 b - 7 the larger half
# has b blocks and the smaller b - 1, so consecutive steps of a record alternate between two limb counts, L = 2 b + 2 = 0 and
# 2 mod 4.  And 1..16 at modulus 10, the smallest count whose larger half has b blocks: many divisions per limb.
SWEEP_B = range(1, 41)


def _sweep(b):
    out = [(65536, max(2, 8 * b - 7)), (65535, max(2, 8 * b - 7))]
    if b <= 16:
        out.append((10, next(c for c in range(2, M.COUNT_MAX + 1) if M.block_count(10, (c + 1) // 2) == b)))
    return out


SWEEP = {b: _sweep(b) for b in SWEEP_B}
SWEEP_SHAPES = [s for b in SWEEP_B for s in SWEEP[b]]


def symbols(rnd, mod, count, oor):
    """count symbols below mod; with oor (and a modulus that leaves room) one to three of them at or above it"""
    s = [rnd.randrange(mod) for _ in range(count)]
    if oor and mod < 65536:
        for _ in range(rnd.randrange(1, 4)):
            s[rnd.randrange(count)] = rnd.randrange(mod, 65536)
    return s


# ---- the committed fixture (tools/make_golden_beltfmt.py writes it from the reference): a row's inputs come from its seed
def fixture_cases():
    out = []
    for j, (mod, count) in enumerate(ALL_SHAPES):
        for k, key_len in enumerate(KEY_LENS):
            for decr in (0, 1):
                out.append({"mod": mod, "count": count, "key_len": key_len, "decr": decr, "iv": (j + k + decr) % 3 != 0,
                            "oor": (j + 2 * k + decr) % 4 == 1, "seed": 7000000 + 1000 * j + 10 * k + decr})
    # the seam shapes, appended (a row's seed comes from its index): one key length each, both directions
    for j, (mod, count) in enumerate(PLAN_SHAPES, len(ALL_SHAPES)):
        k = j % 3
        for decr in (0, 1):
            out.append({"mod": mod, "count": count, "key_len": KEY_LENS[k], "decr": decr, "iv": (j + k + decr) % 3 != 0,
                        "oor": (j + 2 * k + decr) % 4 == 1, "seed": 7000000 + 1000 * j + 10 * k + decr})
    return out


def case_inputs(c):
    rnd = random.Random(c["seed"])
    return {"key": rnd.randbytes(c["key_len"]), "iv": rnd.randbytes(16) if c["iv"] else None,
            "symbols": symbols(rnd, c["mod"], c["count"], c["oor"])}


def encode(syms):
    """what the fixture records of an output: hex of the little-endian u16, or their sha256 above 64 symbols"""
    raw = struct.pack(f"<{len(syms)}H", *syms)
    return raw.hex() if len(syms) <= 64 else "sha256:" + hashlib.sha256(raw).hexdigest()


# bee2's published vectors (STB 34.101.31 A.26; test/crypto/belt_test.c:692-721): key = beltH()[128..160), iv = beltH()[192..208),
# the symbols 0, 1, 2 ..
BEE2_VECTORS = [(10, [6, 9, 3, 4, 7, 7, 0, 3, 5, 2]),
                (58, [7, 4, 6, 21, 49, 55, 24, 23, 22, 50, 27, 39, 24, 24, 17, 32, 57, 43, 26, 5, 29]),
                (65536, [14290, 31359, 58054, 51842, 44653, 34762, 28652, 48929, 6541, 13788, 7784, 46182, 61098, 43056, 3564,
                         21568, 63878])]

# pairs (mod, n) whose block count the fixture records from the reference: the exception, its neighbours, the shapes' halves,
# the ends of the ranges and seeded pairs
def block_pairs():
    pairs = [(49667, 160), (49667, 159), (49667, 161), (49666, 160), (49668, 160), (2, 1), (2, 64), (2, 65), (2, 300), (65536, 1),
             (65536, 300), (65535, 300), (65535, 4), (65535, 5), (256, 8), (256, 9), (257, 8), (3, 300), (10, 19), (10, 20), (58, 10),
             (58, 11)]
    for mod, count in ALL_SHAPES:
        pairs += [(mod, (count + 1) // 2), (mod, count // 2)]
    rnd = random.Random(0xB10C)
    pairs += [(rnd.randrange(2, 65537), rnd.randrange(1, 301)) for _ in range(300)]
    return sorted(set(pairs))


# ---- batches
class Batch:
    def __init__(self, mod, count, n, key_len=32, seed=0, ivs=True, oor=True):
        rnd = random.Random((mod * 1000 + count) * 1000 + n + 131 * key_len + seed)
        self.mod, self.count, self.n = mod, count, n
        self.key = rnd.randbytes(key_len)
        self.ivs = rnd.randbytes(16 * n) if ivs else None
        self.rows = [symbols(rnd, mod, count, oor and i % 5 == 2) for i in range(n)]
        self.records = b"".join(struct.pack(f"<{count}H", *r) for r in self.rows)
        self._want = {}

    def iv(self, i):
        return None if self.ivs is None else self.ivs[16 * i:16 * i + 16]

    def want(self, decr):
        """the model's output for the whole batch in one direction, computed once"""
        if decr not in self._want:
            self._want[decr] = b"".join(struct.pack(f"<{self.count}H", *M.crypt(decr, self.mod, self.rows[i], self.key, self.iv(i)))
                                        for i in range(self.n))
        return self._want[decr]

    def in_range(self, i):
        return all(s < self.mod for s in self.rows[i])


@functools.lru_cache(maxsize=None)
def batch(mod, count, n, key_len=32, seed=0, ivs=True, oor=True):
    return Batch(mod, count, n, key_len, seed, ivs, oor)
