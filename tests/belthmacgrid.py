"""Lengths, fixture rows and batches for belt-hmac / belt-pbkdf2 (bee2_amd/csrc/belt_hmac_kernels.hip).  Inputs come from
seeds; the fixture (tests/golden/belt_hmac.json, written by tools/make_golden_belthmac.py from the reference) holds the
outputs.  No GPU here: tests/test_belthmac.py runs the CPU side, tests/test_gpu_belthmac.py the batches."""
import functools
import random

import orc_belthmac as M

# keys / passwords: empty, short, around the 32 octets up to which a key is zero-padded, and hashed ones of two, exactly
# two, three and four blocks
KEY_LENS = (0, 1, 29, 31, 32, 33, 42, 63, 64, 65, 97)
# messages / salts: every position of the PBKDF2 suffix against a block boundary (27 .. 32 mod 32), several blocks
MSG_LENS = (0, 1, 27, 28, 29, 31, 32, 33, 63, 64, 65, 100, 1000)
ITERS = (1, 2, 3, 50)
BATCH_SIZES = (1, 63, 64, 65, 257)
SALT_LENS = (0, 8, 27, 28, 29, 31, 32, 60)
ITER_CAP = 1 << 17                                 # iterations of one batch launch (HMAC_ITER_MAX, belt_hmac_common.hpp)


def fixture_cases():
    out = []
    for a, key_len in enumerate(KEY_LENS):
        for b, msg_len in enumerate(MSG_LENS):
            out.append({"kind": "hmac", "key_len": key_len, "msg_len": msg_len, "iter": 1, "seed": 7100000 + 100 * a + b})
            for c, it in enumerate(ITERS):
                out.append({"kind": "pbkdf2", "key_len": key_len, "msg_len": msg_len, "iter": it,
                            "seed": 7200000 + 1000 * a + 10 * b + c})
    return out


def case_inputs(c):
    """(key or password, message or salt) of a fixture row"""
    rnd = random.Random(c["seed"])
    return rnd.randbytes(c["key_len"]), rnd.randbytes(c["msg_len"])


def offsets(lens, first=0):
    out = [first]
    for n in lens:
        out.append(out[-1] + n)
    return out


class Batch:
    """n records: key i of key_lens[i % ..] octets, message i of msg_lens[i % ..] octets (both walk their lists at different
    strides, so that a wavefront holds short and hashed keys and every tail residue at once); shared: one key of that many
    octets for all.  want = the 32-octet MACs of the model, computed once"""

    def __init__(self, n, key_lens=KEY_LENS, msg_lens=MSG_LENS, shared=None, seed=0):
        rnd = random.Random(1000 * n + 31 * seed + (0 if shared is None else 7 + shared))
        self.n, self.shared = n, shared
        self.key_lens = [key_lens[(i // len(msg_lens) + i) % len(key_lens)] for i in range(n)]
        self.msg_lens = [msg_lens[i % len(msg_lens)] for i in range(n)]
        self.key = None if shared is None else rnd.randbytes(shared)
        self.keys = [rnd.randbytes(k) for k in self.key_lens]
        self.msgs = [rnd.randbytes(m) for m in self.msg_lens]
        self._want = None

    def key_of(self, i):
        return self.keys[i] if self.key is None else self.key

    def want(self):
        if self._want is None:
            self._want = [M.hmac(self.key_of(i), self.msgs[i]) for i in range(self.n)]
        return self._want


@functools.lru_cache(maxsize=None)
def batch(n, shared=None, seed=0):
    return Batch(n, shared=shared, seed=seed)


@functools.lru_cache(maxsize=None)
def grid_batch(shared=None):
    """every fixture key length x message length, one record each, shuffled: 143 records, three wavefronts, each with short
    and hashed keys and every tail residue; shared: the same messages under one key of that many octets"""
    b = Batch.__new__(Batch)
    rnd = random.Random(0x484D4143)
    pairs = [(k, m) for k in KEY_LENS for m in MSG_LENS]
    rnd.shuffle(pairs)
    b.n, b.shared = len(pairs), shared
    b.key = None if shared is None else random.Random(shared).randbytes(shared)
    b.key_lens, b.msg_lens = [p[0] for p in pairs], [p[1] for p in pairs]
    b.keys = [rnd.randbytes(k) for k in b.key_lens]
    b.msgs = [rnd.randbytes(m) for m in b.msg_lens]
    b._want = None
    return b
