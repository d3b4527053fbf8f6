"""Batches for the ragged hash kernels (bee2_amd/csrc/mixed_kernels.hip, launch_hash_ragged) in which every wanted length
starts at every offset mod 16.  Pure Python, no oracle and no GPU: tests/test_ragged_grid.py proves the coverage on the CPU,
tests/test_gpu_hash_ragged_grid.py and tests/test_gpu_bign_sign.py run the batches.

The short kernels read a block as the aligned 16-octet quads that hold it and shift by p mod 16; the tail masks follow
len mod <block size>; the 8-lane / pair forms shift by p mod 4 and pad by len mod <block size>.  So a length set is crossed with
the 16 start alignments: before each wanted message goes a filler message of 0..15 octets that moves the cursor to the wanted
residue.  Fillers are ordinary messages of the batch -- their digests are checked like any other."""
import random

ALGS = (0, 128, 192, 256)                      # belt-hash, bash256, bash384, bash512 (the `alg` of bee2hip_hash_ragged)
BLOCK = {0: 32, 128: 128, 192: 96, 256: 64}    # octets per compression / sponge rate
DIGEST = {0: 32, 128: 32, 192: 48, 256: 64}
LONG_FROM = 4096                               # RAGGED_LONG: messages from this length on go to the 8-lane / pair kernels


def short_lengths(alg):
    """0 .. B+17 (every tail length and the first block boundary, across a quad), then around two and three blocks"""
    B = BLOCK[alg]
    return list(range(0, B + 18)) + [2 * B - 1, 2 * B, 2 * B + 1] + list(range(3 * B - 16, 3 * B + 2))


def long_lengths(alg):
    """4095 (the last length the short kernel owns), then the long forms: whole blocks, one octet either side, the 32-octet
    steps of the belt-hash prefetch, one rate block past 4096 and two 4 KiB"""
    B = BLOCK[alg]
    want = [4095, 4096, 4097, 4096 + 31, 4096 + 32, 4096 + 33, 4096 + B - 1, 4096 + B, 4096 + B + 1, 8191, 8192, 8193]
    return sorted(set(want))


def build(lengths, seed, extra=()):
    """-> (blob, offsets): messages packed back to back, message i = blob[offsets[i]:offsets[i + 1]].

    For every L of `lengths` and every s in 0..15, in that order, a filler of (s - cursor) mod 16 octets and then a message of
    L octets starting at an offset = s mod 16.  `extra`: lengths of further messages (any length, any place) spread evenly
    between the (filler, message) pairs -- the short traffic and the empty padding of the large-batch cases.  Contents are
    random.Random(seed) octets."""
    rnd = random.Random(seed)
    pairs = [(L, s) for L in lengths for s in range(16)]
    extra = list(extra)
    lens = []
    cursor, taken = 0, 0
    for k, (L, s) in enumerate(pairs):
        upto = len(extra) * (k + 1) // (len(pairs) + 1)          # (the rest goes behind the last pair)
        for e in extra[taken:upto]:
            lens.append(e)
            cursor += e
        taken = upto
        f = (s - cursor) % 16
        lens.append(f)
        lens.append(L)
        cursor += f + L
    lens.extend(extra[taken:])
    offsets = [0]
    for n in lens:
        offsets.append(offsets[-1] + n)
    return rnd.randbytes(offsets[-1]), offsets


REGIME_SHORT = 2000                            # messages of 1..199 octets beside the chains in a size-regime batch


def regime_batch(alg, n, seed):
    """the long grid of `alg` inside a batch of exactly n messages: REGIME_SHORT messages of 1..199 octets and empty messages
    (which move no cursor) fill it up, shuffled among themselves"""
    rnd = random.Random(seed ^ 0x5EED)
    grid = 2 * 16 * len(long_lengths(alg))
    assert n >= grid + REGIME_SHORT
    extra = [rnd.randrange(1, 200) for _ in range(REGIME_SHORT)] + [0] * (n - grid - REGIME_SHORT)
    rnd.shuffle(extra)
    blob, offsets = build(long_lengths(alg), seed, extra)
    assert len(offsets) == n + 1
    return blob, offsets


def coverage(offsets):
    """the set of (start mod 16, length) over all messages of a batch"""
    return {(offsets[i] % 16, offsets[i + 1] - offsets[i]) for i in range(len(offsets) - 1)}


def missing(offsets, lengths):
    """(s, L) pairs of the grid that the batch lacks: must be empty"""
    have = coverage(offsets)
    return sorted((s, L) for L in lengths for s in range(16) if (s, L) not in have)


def chunks(n, chunk):
    """a batch of n messages cut into launches of at most `chunk`: (first, count), every message in exactly one (the offsets stay
    absolute, so no message changes its alignment)"""
    return [(lo, min(chunk, n - lo)) for lo in range(0, n, chunk)]


# ---- the secret launch behind bee2hip_bignSign2_batch (capi_bign.hip, sign_batch_host): additional input of more than 64 octets
# makes the host assemble oid || d || t per item, ml = oid_len + l/4 + t_len octets each, item i at i * ml
SIGN_N = 67
SIGN_OID_LEN = 11                               # the DER OIDs of bee2_amd.engine.LEVEL_OID
SIGN_T_SHARED = (1, 31, 32, 33, 63, 64, 65, 96, 97, 300, 4097, 5000)
SIGN_T_ODD = {128: 66, 192: 70, 256: 130}       # one t_len per level with ml odd (109, 129, 205): item i starts at i * ml
SIGN_T_DEV = (1, 31, 32, 33, 63, 64)            # the device entry assembles the message itself: t_len <= 64


def sign_ml(l, t_len):
    return SIGN_OID_LEN + l // 4 + t_len


def sign_alignments(l, t_len, n=SIGN_N):
    return {(i * sign_ml(l, t_len)) % 16 for i in range(n)}
