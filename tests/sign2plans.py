"""Batches for bee2hip_bignSign2_batch on parameter sets whose q rejects one-time-key draws (bign_sign_nonce_kernel's loop,
bign_sign_kernels.hip): which private key and hash sits in which lane, with the one-time key and the number of passes the
MODEL (tests/orc_sign2.py on the C oracle's belt-hash / belt-wbl) says each lane takes.  One lane per item, 64 lanes per
wavefront, so item i runs in wavefront i // 64 at lane i % 64, and a wavefront loops as long as its slowest lane.

No GPU here: tests/test_sign2_model.py proves on the CPU that every batch holds the mix of pass counts its name promises,
tests/test_gpu_bign_sign2_loop.py runs them.  Batches are filled by filtering a seeded stream of candidates by pass count;
with one rejection in two that is instant.  Everything is cached: a plan is computed once and never changed."""
import functools
import json
import os
import random
from collections import namedtuple

import orc_generic as OG
import orc_sign2 as S2
import orclib

HERE = os.path.dirname(os.path.abspath(__file__))
AFIX = json.load(open(os.path.join(HERE, "golden", "bign_generic_adv.json")))
NFIX = json.load(open(os.path.join(HERE, "golden", "bign_sign2_nonce.json")))
OIDS = [bytes.fromhex(o) for o in NFIX["oids"]]            # DER lengths 0, 1, 2, 3 (mod 4)
LEVELS = (128, 192, 256)
T_DEVICE = (0, 1, 31, 32, 33, 64)                          # theta hashed by the nonce kernel itself
T_HOSTED = (65, 200)                                       # theta from the ragged belt-hash launch (theta_in)
MIXED_N = (1, 63, 64, 65, 257, 1025)
EDGE_LANES = (0, 31, 32, 63)
HALF, LOW1, RANDOM_ODD, ONES = "2^(2l-1) + 1", "low limb 1", "random odd", "2^(2l) - 1"

# one lane: d, h octets; k the model's one-time key (int; None where d is refused); passes the model's count for the lane,
# refused or not -- the kernel's loop does not look at d
Item = namedtuple("Item", "d h k passes")
Batch = namedtuple("Batch", "name si l oid t items")


def set_indices(l, q_kind, kind="adv"):
    return [i for i, s in enumerate(AFIX["sets"]) if s["l"] == l and s["q_kind"] == q_kind and s["kind"] == kind]


def q_of(si):
    return OG.le(bytes.fromhex(AFIX["sets"][si]["q"]))


@functools.lru_cache(None)
def _orc():
    return orclib.load()


def model_item(oid, t, d, h, q):
    orc = _orc()
    k, passes = S2.nonce(oid, d, t, h, q, orc.belt_hash, orc.wbl)
    return Item(d, h, k if 0 < OG.le(d) < q else None, passes)


class _Stream:
    """seeded candidates for one (set, oid, t): take(pred) hands out the next one whose pass count fits"""

    def __init__(self, si, oid, t, seed):
        self.q, self.no = q_of(si), AFIX["sets"][si]["l"] // 4
        self.oid, self.t, self.rnd = oid, t, random.Random(seed)

    def take(self, pred=None, d=None, h=None):
        """d, h: fixed integers or None for a fresh draw (hashes from the whole of [0, 2^(2l)): about half are >= q on a
        q near 2^(2l-1))"""
        enc = lambda v: v.to_bytes(self.no, "little")
        for _ in range(100000):
            it = model_item(self.oid, self.t, enc(self.rnd.randrange(1, self.q) if d is None else d),
                            enc(self.rnd.getrandbits(8 * self.no) if h is None else h), self.q)
            if pred is None or pred(it.passes):
                return it
            assert d is None or h is None, "a fixed lane cannot be filtered"
        raise AssertionError("no candidate")


def refused_keys(si):
    l = AFIX["sets"][si]["l"]
    return (0, q_of(si), (1 << (2 * l)) - 1)


@functools.lru_cache(None)
def mixed(l, n):
    """the q = 2^(2l-1) + 1 set: every full wavefront w has a 1-pass lane at (7 w + 3) % 64 and a lane with >= 4 passes at
    (11 w + 40) % 64 (4 w + 37 is odd: the two never meet); n = 1 is one item with >= 4 passes; the last item of n = 65 has
    >= 5, alone in its wavefront.  From n = 63 on, wavefront 0 also holds H = q, H = q + 1, H = 0, H = q - 1, H = 2^(2l) - 1
    (lanes 5..9), the three refused keys (lanes 20..22) and an item with >= 6 passes (lane 30); every other lane is a plain
    draw."""
    si = set_indices(l, HALF)[0]
    q = q_of(si)
    S = _Stream(si, OIDS[l // 64 % 4], None, 0x3100 + l + n)
    spec = {}
    if n == 1:
        spec[0] = dict(pred=lambda p: p >= 4)
    for w in range(n // 64):
        spec[64 * w + (7 * w + 3) % 64] = dict(pred=lambda p: p == 1)
        spec[64 * w + (11 * w + 40) % 64] = dict(pred=lambda p: p >= 4)
    if n >= 63:
        for lane, hv in zip(range(5, 10), (q, q + 1, 0, q - 1, (1 << (2 * l)) - 1)):
            spec[lane] = dict(h=hv)
        for lane, dv in zip(range(20, 23), refused_keys(si)):
            spec[lane] = dict(d=dv)
        spec[30] = dict(pred=lambda p: p >= 6)
    if n == 65:
        spec[64] = dict(pred=lambda p: p >= 5)
    return Batch(f"mixed l={l} n={n}", si, l, S.oid, None, tuple(S.take(**spec.get(i, {})) for i in range(n)))


def _one_odd_lane(name, l, lane, odd, rest, seed):
    """n = 64: `lane` fits `odd`, every other lane fits `rest`; a refused key (d = 0 / q / 2^(2l) - 1 by lane) sits two lanes
    further on and loops like its neighbours"""
    si = set_indices(l, HALF)[1]
    S = _Stream(si, OIDS[(l // 64 + 1) % 4], None, seed + 64 * l + lane)
    bad = (lane + 2) % 64
    dv = refused_keys(si)[EDGE_LANES.index(lane) % 3]
    return Batch(f"{name} l={l} lane={lane}", si, l, S.oid, None,
                 tuple(S.take(odd) if i == lane else S.take(rest, d=dv if i == bad else None) for i in range(64)))


@functools.lru_cache(None)
def straggler(l, lane):
    """one wavefront in which `lane` alone needs >= 5 passes, every other lane 1"""
    return _one_odd_lane("straggler", l, lane, lambda p: p >= 5, lambda p: p == 1, 0x57A6)


@functools.lru_cache(None)
def early_bird(l, lane):
    """one wavefront in which `lane` alone has its k after 1 pass and has to keep it while every other lane takes >= 3"""
    return _one_odd_lane("early bird", l, lane, lambda p: p == 1, lambda p: p >= 3, 0xEA51)


@functools.lru_cache(None)
def q_kind_batch(si):
    """130 plain draws on set si, the refused keys at items 64..66 (the second wavefront); where q rejects at all, lane 40 of
    each full wavefront takes 1 pass and lane 3 takes >= 3"""
    s = AFIX["sets"][si]
    S = _Stream(si, OIDS[si % 4], None, 0x9B00 + si)
    bad = dict(zip((64, 65, 66), refused_keys(si)))
    pred = {} if s["q_kind"] == ONES else {3: lambda p: p >= 3, 40: lambda p: p == 1}
    return Batch(f"{s['q_kind']} set {si}", si, s["l"], S.oid, None,
                 tuple(S.take(pred.get(i % 64) if i < 128 else None, d=bad.get(i)) for i in range(130)))


@functools.lru_cache(None)
def theta_batch(l, t_len, oid_i):
    """n = 65 on the "low limb 1" set with a shared additional input of t_len octets and the OID of length oid_i (mod 4);
    item 64 takes >= 3 passes, item 7 has a refused key"""
    si = set_indices(l, LOW1)[0]
    t = random.Random(0x7400 + t_len).randbytes(t_len) if t_len else None
    S = _Stream(si, OIDS[oid_i], t, 0x7E00 + 1000 * oid_i + t_len + l)
    return Batch(f"theta l={l} t={t_len} oid%4={oid_i}", si, l, S.oid, t,
                 tuple(S.take(d=0) if i == 7 else S.take((lambda p: p >= 3) if i == 64 else None) for i in range(65)))


def wavefronts(b):
    """pass counts of the FULL wavefronts of a batch"""
    p = [it.passes for it in b.items]
    return [p[i:i + 64] for i in range(0, len(p) - 63, 64)]
