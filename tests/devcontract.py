"""The device-pointer API (include/bee2hip.h section 3) as data: one record per single-device bee2hip_*_dev entry and
mode.  A record knows how to make a call's buffers and host arguments from (size, seed), how to make the call through
bee2_amd.engine on device tensors, and what every output buffer must hold afterwards -- computed with tests/orclib.py
(and plain integer arithmetic in GF(2^128)) alone.  tests/test_gpu_dev_contract.py runs every record against its range,
alignment, aliasing and stream-capture contract; tests/test_dev_contract_registry.py checks on the CPU that no _dev entry
of the header is without a record.

Importable without a GPU and without torch (the call functions only touch the tensors they are handed)."""
import functools
import os
import re
import struct

import numpy as np

from bee2_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bee2hip.h")

GUARD = 4096                               # bytes of seeded pattern kept on each side of every buffer
OFFSETS16 = (16, 48, 112, 240)             # base + off is 16 mod 32, 64, 128, 256 in turn

# the orchestrators over several devices: they call the single-device entries on each device's shard and are tested in
# tests/test_gpu_multi.py; their shards are whole allocations of other devices, not ranges of one
EXEMPT = {
    "bee2hip_bashF_batch_multi_dev": "multi-device orchestrator over bee2hip_bashF_batch_dev (test_gpu_multi.py)",
    "bee2hip_beltCTR_blocks_multi_dev": "multi-device orchestrator over bee2hip_beltCTR_blocks_dev (test_gpu_multi.py)",
    "bee2hip_bignVerifyL_batch_multi_dev": "multi-device orchestrator over bee2hip_bignVerifyL_batch_dev (test_gpu_multi.py)",
    "bee2hip_bignVerifyL_onekey_batch_multi_dev": "multi-device orchestrator over the one-signer entry (test_gpu_multi.py)",
    "bee2hip_bignVerifyL_keyed_batch_multi_dev": "multi-device orchestrator over the keyed entry (test_gpu_multi.py)",
    "bee2hip_bashHash_beltMAC_batch_multi_dev": "multi-device orchestrator over the fused entry (test_gpu_multi.py)",
}


def header_dev_symbols():
    with open(HEADER) as f:
        return set(re.findall(r"\b(bee2hip_\w+_dev)\s*\(", f.read()))


# ------------------------------------------------------------------------------------------------ GF(2^128), plain integers
POLY = (1 << 128) | 0x87


def gf_mul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a <<= 1
        if a >> 128:
            a ^= POLY
        b >>= 1
    return r


def gf_xpow(e):
    base, r = 2, 1
    while e:
        if e & 1:
            r = gf_mul(r, base)
        base = gf_mul(base, base)
        e >>= 1
    return r


Q_INV = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFF82            # (x + 1)^-1


def bde_state(s0, j):
    """s0 * x^j: the belt-bde tweak j blocks into the stream"""
    return gf_mul(s0, gf_xpow(j))


def che_state(s0, j):
    """S_j of S <- S*x ^ 1 from S_0: S_0 x^j ^ (x^j ^ 1) / (x ^ 1)"""
    p = gf_xpow(j)
    return gf_mul(s0, p) ^ gf_mul(p ^ 1, Q_INV)


def horner(t, r, data):
    """t <- (t ^ X) * r over the 16-byte blocks X of data, the last one zero-padded (belt_dwp.c:96-101); the product with the
    fixed r through 16 tables of 256 entries (r * byte * x^(8 i)), so that 2^16 blocks stay under a second"""
    tabs = []
    for i in range(16):
        one = [gf_mul(r, 1 << (8 * i + b)) for b in range(8)]
        tab = [0] * 256
        for v in range(1, 256):
            low = v & -v
            tab[v] = tab[v ^ low] ^ one[low.bit_length() - 1]
        tabs.append(tab)
    for off in range(0, len(data), 16):
        x = t ^ int.from_bytes(data[off:off + 16].ljust(16, b"\0"), "little")
        t = 0
        for i in range(16):
            t ^= tabs[i][(x >> (8 * i)) & 0xFF]
    return t


# ------------------------------------------------------------------------------------------------ records
class Buf:
    """one device buffer of a call: its bytes on entry, the alignment the header grants it (16: placed at every offset of
    OFFSETS16; 8 / 4 / 1: placed at exactly that offset from a 256-byte boundary), and whether the entry may write it"""

    def __init__(self, name, data, align=16, out=False):
        self.name, self.data, self.align, self.out = name, bytes(data), align, out


class Case:
    def __init__(self, bufs, **args):
        self.bufs, self.args = bufs, args

    def __getitem__(self, name):
        for b in self.bufs:
            if b.name == name:
                return b.data
        raise KeyError(name)

    @property
    def nbytes(self):
        return sum(len(b.data) for b in self.bufs)


class Record:
    """make(orc, size, seed) -> Case, with host arguments that depend on the size only (a captured call bakes them in);
    call(eng, T, case) with T = {buffer name: uint8 device tensor}; expect(orc, case) -> {output buffer: bytes, or a list of
    (offset, bytes) where the oracle is sampled}.  capture = the size a stream capture is tried with, or None with why_not."""

    def __init__(self, name, entry, sizes, make, call, expect, capture=None, why_not=None):
        assert (capture is None) != (why_not is None)
        self.name, self.entry, self.sizes, self.make, self.call, self.expect = name, entry, sizes, make, call, expect
        self.capture, self.why_not = capture, why_not


def resolve(size, cus):
    """block counts around the persistent-grid cap are named, not numbered: the cap depends on the card.  launch_ctr_t,
    launch_modes_t, launch_belt_bde and launch_belt_che start at most CUs * (BeltTabWide::kBytes / CtrTab::kBytes) workgroups
    -- the wide table is 16 KiB, the CTR one 8 KiB: two workgroups per CU -- of CTR_WG = 1024 lanes, one block per lane and
    pass: above cap = CUs * 2 * 1024 blocks every workgroup loops"""
    cap = cus * 2 * 1024
    named = {"cap-1": cap - 1, "cap": cap, "cap+1": cap + 1, "2cap+65": 2 * cap + 65}
    if isinstance(size, tuple):
        return tuple(named.get(s, s) for s in size)
    return named.get(size, size)


def edges(*units):
    out = {1}
    for u in units:
        out |= {u - 1, u, u + 1}
    return sorted(out)


BLOCK_SIZES = edges(64, 1024) + ["cap-1", "cap", "cap+1", "2cap+65"]
BIGN_SIZES = [1, 63, 64, 65, 255, 256, 257, 1025]
BIGN_WIDE_SIZES = [1, 65, 257]             # signing-side records on the wider curves, beyond the levels the entries are held to: oracle time
KEY = bytes(range(0x40, 0x60))
IV = bytes(range(0xA0, 0xB0))


def _codes(codes):
    return struct.pack(f"<{len(codes)}I", *codes)


@functools.lru_cache(maxsize=None)
def _golden():
    import orclib
    return orclib.Golden()


# ---- bashF
def _bashF():
    def make(orc, n, seed):
        return Case([Buf("states", orc.fill(192 * n, seed), 16, True)])

    def call(eng, T, c):
        eng.bashF_batch_dev(T["states"])

    def expect(orc, c):
        return {"states": orc.bashF_batch(c["states"], nthreads=8)}
    return [Record("bashF", "bee2hip_bashF_batch_dev", edges(32, 64, 256) + [4097], make, call, expect, capture=257)]


# ---- belt: CTR, E_K, ECB / CBC, BDE, CHE, SDE, the CBC batch, the authenticator
def _belt_blocks():
    recs = []

    def ctr_make(orc, n, seed):
        kw, c0 = orc.ctr_start(KEY, IV)
        return Case([Buf("buf", orc.fill(16 * n, seed), 16, True)], kw=kw, c0=c0, first=5)

    def ctr_call(eng, T, c):
        eng.beltCTR_blocks_dev(T["buf"], c.args["kw"], c.args["c0"], c.args["first"])

    def ctr_expect(orc, c):
        want = np.frombuffer(c["buf"], dtype=np.uint8).copy()
        orc.ctr_blocks_np(want, c.args["kw"], c.args["c0"], first=c.args["first"], nthreads=8)
        return {"buf": want.tobytes()}
    recs.append(Record("ctr", "bee2hip_beltCTR_blocks_dev", BLOCK_SIZES, ctr_make, ctr_call, ctr_expect, capture=1025))

    def enc_make(orc, n, seed):
        return Case([Buf("blocks", orc.fill(16 * n, seed), 16, True)], kw=bytes(orc.key_expand(KEY)))

    def enc_call(eng, T, c):
        eng.beltBlockEncr_dev(T["blocks"], c.args["kw"])

    def enc_expect(orc, c):
        return {"blocks": orc.ecb(c["blocks"], KEY)[1]}
    recs.append(Record("block_encr", "bee2hip_beltBlockEncr_dev", edges(64, 1024), enc_make, enc_call, enc_expect, capture=1025))

    for name, mode in (("ecb_e", 0), ("ecb_d", 1), ("cbc_d", 2)):
        def make(orc, n, seed, mode=mode):
            return Case([Buf("src", orc.fill(16 * n, seed)), Buf("dst", orc.fill(16 * n, seed ^ 0x5A5A), 16, True)],
                        mode=mode, kw=bytes(orc.key_expand(KEY)), iv=IV if mode == 2 else None)

        def call(eng, T, c):
            eng.beltModes_blocks_dev(c.args["mode"], T["src"], T["dst"], c.args["kw"], c.args["iv"])

        def expect(orc, c):
            m = c.args["mode"]
            return {"dst": orc.cbc(c["src"], KEY, IV, True)[1] if m == 2 else orc.ecb(c["src"], KEY, m == 1)[1]}
        recs.append(Record(name, "bee2hip_beltModes_blocks_dev", BLOCK_SIZES, make, call, expect, capture=1025))

    far = [(65, 63), (65, (1 << 32) - 1), (1025, 63), (1025, (1 << 32) - 1)]
    for name, decr in (("bde_e", 0), ("bde_d", 1)):
        def make(orc, size, seed, decr=decr):
            n, first = size if isinstance(size, tuple) else (size, 0)
            return Case([Buf("src", orc.fill(16 * n, seed)), Buf("dst", orc.fill(16 * n, seed ^ 0x5A5A), 16, True),
                         Buf("s_out", orc.fill(16, seed ^ 0x77), 4, True)],
                        decr=decr, kw=bytes(orc.key_expand(KEY)), s0=orc.block_encr(IV, KEY), first=first)

        def call(eng, T, c):
            eng.beltBDE_blocks_dev(c.args["decr"], T["src"], T["dst"], c.args["kw"], c.args["s0"], c.args["first"], T["s_out"])

        def expect(orc, c):
            s = bde_state(int.from_bytes(c.args["s0"], "little"), c.args["first"]).to_bytes(16, "little")
            out, after = orc.bde_blocks_from(c["src"], KEY, s, bool(c.args["decr"]))
            return {"dst": out, "s_out": after}
        recs.append(Record(name, "bee2hip_beltBDE_blocks_dev", BLOCK_SIZES + far, make, call, expect, capture=1025))

    def che_make(orc, size, seed):
        n, first = size if isinstance(size, tuple) else (size, 0)
        return Case([Buf("src", orc.fill(16 * n, seed)), Buf("dst", orc.fill(16 * n, seed ^ 0x5A5A), 16, True),
                     Buf("s_out", orc.fill(16, seed ^ 0x77), 4, True)],
                    kw=bytes(orc.key_expand(KEY)), s0=orc.block_encr(IV, KEY), first=first)

    def che_call(eng, T, c):
        eng.beltCHE_blocks_dev(T["src"], T["dst"], c.args["kw"], c.args["s0"], c.args["first"], T["s_out"])

    def che_expect(orc, c):
        s = che_state(int.from_bytes(c.args["s0"], "little"), c.args["first"]).to_bytes(16, "little")
        out, after = orc.che_blocks_from(c["src"], KEY, s)
        return {"dst": out, "s_out": after}
    recs.append(Record("che", "bee2hip_beltCHE_blocks_dev", BLOCK_SIZES + far, che_make, che_call, che_expect, capture=1025))
    return recs


def _belt_sde():
    recs = []
    sizes = [(nb, ns) for nb in (2, 3, 15, 16, 17, 24, 32) for ns in (1, 1023, 1024, 1025)]
    for name, decr in (("sde_e", 0), ("sde_d", 1)):
        def make(orc, size, seed, decr=decr):
            nb, ns = size
            return Case([Buf("sectors", orc.fill(16 * nb * ns, seed), 16, True), Buf("ivs", orc.fill(16 * ns, seed ^ 0x1111))],
                        decr=decr, sector_bytes=16 * nb, kw=bytes(orc.key_expand(KEY)))

        def call(eng, T, c):
            eng.beltSDE_sectors_dev(c.args["decr"], T["sectors"], c.args["sector_bytes"], c.args["kw"], T["ivs"])

        def expect(orc, c):
            sb, data, ivs = c.args["sector_bytes"], c["sectors"], c["ivs"]
            ns = len(data) // sb
            step = max(1, ns // 40)               # the oracle is quadratic per sector: first, last, every ceil(n / 40)-th at least
            segs = []
            for i in sorted(set(range(0, ns, step)) | {ns - 1}):
                segs.append((i * sb, orc.sde(data[i * sb:(i + 1) * sb], KEY, ivs[16 * i:16 * i + 16], bool(c.args["decr"]))[1]))
            return {"sectors": segs}
        recs.append(Record(name, "bee2hip_beltSDE_sectors_dev", sizes, make, call, expect, capture=(16, 1025)))
    return recs


def _belt_cbc_batch():
    def make(orc, size, seed):
        nblk, n = size
        return Case([Buf("msgs", orc.fill(16 * nblk * n, seed), 16, True), Buf("ivs", orc.fill(16 * n, seed ^ 0x2222), 16, True)],
                    nblk=nblk, kw=bytes(orc.key_expand(KEY)))

    def call(eng, T, c):
        eng.beltCBCEncr_batch_dev(T["msgs"], c.args["nblk"], c.args["kw"], T["ivs"])

    def expect(orc, c):
        mb = 16 * c.args["nblk"]
        out = [orc.cbc(c["msgs"][i * mb:(i + 1) * mb], KEY, c["ivs"][16 * i:16 * i + 16])[1] for i in range(len(c["ivs"]) // 16)]
        return {"msgs": b"".join(out), "ivs": b"".join(o[-16:] for o in out)}
    sizes = [(nblk, n) for nblk in (1, 2, 17) for n in (1, 1023, 1024, 1025)]
    return [Record("cbc_batch", "bee2hip_beltCBCEncr_batch_dev", sizes, make, call, expect, capture=(17, 1025))]


def _belt_dwp():
    def make(orc, nbytes, seed):
        r, t = orc.block_encr(orc.block_encr(IV, KEY), KEY), bytes(range(16, 32))
        # nothing but the nbytes belongs to the call: what lies behind them is guard pattern, so the zero padding of the last
        # block has to come from the kernel
        return Case([Buf("data", orc.fill(nbytes, seed)), Buf("t_out", orc.fill(16, seed ^ 0x33), 4, True)], nbytes=nbytes, r=r, t=t)

    def call(eng, T, c):
        eng.beltDWP_absorb_dev(T["data"], c.args["nbytes"], c.args["r"], c.args["t"], T["t_out"])

    def expect(orc, c):
        t = horner(int.from_bytes(c.args["t"], "little"), int.from_bytes(c.args["r"], "little"), c["data"])
        return {"t_out": t.to_bytes(16, "little")}
    sizes = [0, 1, 15, 16, 17, 16383, 16384, 16385, (1 << 20) + 5]
    return [Record("dwp_absorb", "bee2hip_beltDWP_absorb_dev", sizes, make, call, expect, capture=16385)]


# ---- bign
def _tiled(rows, n, start):
    reps = (start % len(rows) + n) // len(rows) + 1
    return (rows * reps)[start % len(rows): start % len(rows) + n]


def _verify_triples(l):
    g = _golden()
    if l == 128:
        return g.bign_base
    return [tuple(bytes.fromhex(t[k]) for k in ("hash", "sig", "pubkey")) for t in g.bign_big[str(l)]["base"]]


def _damage(rows, seed, width):
    """a few rows get one flipped bit (at least one when there are four rows or more): the codes are not all zero"""
    rng = np.random.default_rng(seed)
    rows = [bytearray(r) for r in rows]
    for i in rng.choice(len(rows), len(rows) // 40 + (len(rows) >= 4), replace=False):
        rows[int(i)][int(rng.integers(0, width))] ^= 1 << int(rng.integers(0, 8))
    return [bytes(r) for r in rows]


def _bign_verify():
    recs = []

    def make_for(l):
        def make(orc, n, seed):
            tr = _tiled(_verify_triples(l), n, seed * 7)
            sigs = _damage([t[1] for t in tr], seed, 3 * l // 8)
            return Case([Buf("hashes", b"".join(t[0] for t in tr)), Buf("sigs", b"".join(sigs)), Buf("pubkeys", b"".join(t[2] for t in tr)),
                         Buf("codes", orc.fill(4 * n, seed ^ 0x44), 4, True)], l=l, oid=E.LEVEL_OID[l])
        return make

    def expect(orc, c):
        return {"codes": _codes(orc.verify_batch_l(c.args["l"], c.args["oid"], c["hashes"], c["sigs"], c["pubkeys"], nthreads=8))}

    recs.append(Record("verify128_fixed_oid", "bee2hip_bign128Verify_batch_dev", BIGN_SIZES, make_for(128),
                       lambda eng, T, c: eng.bign128Verify_batch_dev(T["hashes"], T["sigs"], T["pubkeys"], T["codes"]), expect, capture=257))
    recs.append(Record("verify128_oid", "bee2hip_bignVerify_batch_dev", BIGN_SIZES, make_for(128),
                       lambda eng, T, c: eng.bignVerify_batch_dev(c.args["oid"], T["hashes"], T["sigs"], T["pubkeys"], T["codes"]), expect,
                       capture=257))
    for l in (128, 192, 256):
        recs.append(Record(f"verifyL_{l}", "bee2hip_bignVerifyL_batch_dev", BIGN_SIZES, make_for(l),
                           lambda eng, T, c: eng.bignVerifyL_batch_dev(c.args["l"], c.args["oid"], T["hashes"], T["sigs"], T["pubkeys"], T["codes"]),
                           expect, capture=257))
    return recs


def privkey(orc, l, seed):
    d = bytearray(orc.fill(l // 4, seed))
    d[-1] &= 0x3F
    return bytes(d)


@functools.lru_cache(maxsize=None)
def signed_pool(l, keyseed, count=1025):
    """count valid signatures of seeded hashes under the private key of keyseed, by the oracle: (pubkey, [(hash, sig)])"""
    import orclib
    orc = orclib.load()
    no = l // 4
    d = privkey(orc, l, keyseed)
    code, pub = orc.pubkey_calc(l, d)
    assert code == 0
    hs = orc.fill(no * count, keyseed + 1)
    rows = []
    for i in range(count):
        code, sig = orc.sign2(l, E.LEVEL_OID[l], hs[no * i:no * (i + 1)], d)
        assert code == 0
        rows.append((hs[no * i:no * (i + 1)], sig))
    return pub, rows


KEYSEEDS = (0x1C01, 0x1C02, 0x1C03, 0x1C04, 0x1C05)


def onekey_case(orc, l, n, seed, keyseed=KEYSEEDS[0], pool=1025):
    pub, rows = signed_pool(l, keyseed, pool)
    rows = _tiled(rows, n, seed * 11)
    sigs = _damage([r[1] for r in rows], seed, 3 * l // 8)
    return Case([Buf("hashes", b"".join(r[0] for r in rows)), Buf("sigs", b"".join(sigs)), Buf("codes", orc.fill(4 * n, seed ^ 0x44), 4, True)],
                l=l, oid=E.LEVEL_OID[l], pubkey=pub)


def onekey_call(eng, T, c):
    eng.bignVerifyL_onekey_batch_dev(c.args["l"], c.args["oid"], T["hashes"], T["sigs"], c.args["pubkey"], T["codes"])


def onekey_expect(orc, c):
    n = len(c["codes"]) // 4
    return {"codes": _codes(orc.verify_batch_l(c.args["l"], c.args["oid"], c["hashes"], c["sigs"], c.args["pubkey"] * n, nthreads=8))}


def keyed_case(orc, l, n, nkeys, seed):
    pools = [signed_pool(l, ks, 1025) for ks in KEYSEEDS[:nkeys]]
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, nkeys, n).astype(np.uint32)
    rows = [pools[int(k)][1][(i + seed * 11) % 1025] for i, k in enumerate(idx)]
    sigs = _damage([r[1] for r in rows], seed, 3 * l // 8)
    if n >= 63:
        idx[int(rng.integers(0, n))] = nkeys + 1000           # an index out of range: ERR_BAD_INPUT for that signature
    return Case([Buf("hashes", b"".join(r[0] for r in rows)), Buf("sigs", b"".join(sigs)), Buf("key_index", idx.tobytes(), 4),
                 Buf("codes", orc.fill(4 * n, seed ^ 0x44), 4, True)], l=l, oid=E.LEVEL_OID[l], pubkeys=b"".join(p[0] for p in pools))


def keyed_call(eng, T, c):
    import torch
    eng.bignVerifyL_keyed_batch_dev(c.args["l"], c.args["oid"], T["hashes"], T["sigs"], c.args["pubkeys"], T["key_index"].view(torch.int32),
                                    T["codes"])


def keyed_expect(orc, c):
    l = c.args["l"]
    kb = l // 2
    idx = np.frombuffer(c["key_index"], dtype=np.uint32)
    nkeys = len(c.args["pubkeys"]) // kb
    keys = b"".join(c.args["pubkeys"][kb * int(k):kb * int(k) + kb] if k < nkeys else c.args["pubkeys"][:kb] for k in idx)
    codes = orc.verify_batch_l(l, c.args["oid"], c["hashes"], c["sigs"], keys, nthreads=8)
    return {"codes": _codes([E.ERR_BAD_INPUT if k >= nkeys else code for k, code in zip(idx, codes)])}


def _bign_onekey_keyed():
    recs = [Record("verify_onekey_128", "bee2hip_bignVerifyL_onekey_batch_dev", BIGN_SIZES,
                   lambda orc, n, seed: onekey_case(orc, 128, n, seed), onekey_call, onekey_expect, capture=257),
            Record("verify_keyed_128", "bee2hip_bignVerifyL_keyed_batch_dev", [(n, k) for k in (1, 5) for n in BIGN_SIZES],
                   lambda orc, size, seed: keyed_case(orc, 128, size[0], size[1], seed), keyed_call, keyed_expect,
                   why_not="uploads the keys and the tables' addresses from pageable memory and waits for the copy on every call: refused")]
    return recs


def _bign_keys_and_signing():
    recs = []
    for l in (128, 192, 256):
        def val_make(orc, n, seed, l=l):
            keys = _tiled([bytes.fromhex(c["pubkey"]) for c in _golden().bign_pubkey_val[str(l)]], n, seed * 5)
            return Case([Buf("pubkeys", b"".join(_damage(keys, seed, l // 2))), Buf("codes", orc.fill(4 * n, seed ^ 0x44), 4, True)], l=l)
        recs.append(Record(f"pubkey_val_{l}", "bee2hip_bignPubkeyValL_batch_dev", BIGN_SIZES, val_make,
                           lambda eng, T, c: eng.bignPubkeyValL_batch_dev(c.args["l"], T["pubkeys"], T["codes"]),
                           lambda orc, c: {"codes": _codes(orc.pubkey_val_batch(c.args["l"], c["pubkeys"]))}, capture=257))

    def privs(orc, l, n, seed):
        """n private keys; a few refused ones (0, q and above) so that the codes are not all zero"""
        no = l // 4
        raw = orc.fill(no * n, seed)
        rows = []
        for i in range(n):
            d = bytearray(raw[no * i:no * (i + 1)])
            d[-1] &= 0x3F
            rows.append(bytes(d))
        rng = np.random.default_rng(seed)
        for j, i in enumerate(rng.choice(n, n // 40 + (n >= 4), replace=False)):
            rows[int(i)] = bytes(no) if j % 2 == 0 else b"\xff" * no
        return rows

    for l in (128, 192, 256):
        def calc_make(orc, n, seed, l=l):
            return Case([Buf("privkeys", b"".join(privs(orc, l, n, seed)), 4), Buf("pubkeys", orc.fill(l // 2 * n, seed ^ 0x55), 4, True),
                         Buf("codes", orc.fill(4 * n, seed ^ 0x44), 4, True)], l=l)

        def calc_expect(orc, c):
            l = c.args["l"]
            no = l // 4
            res = [orc.pubkey_calc(l, c["privkeys"][no * i:no * (i + 1)]) for i in range(len(c["privkeys"]) // no)]
            return {"pubkeys": b"".join(p if code == 0 else bytes(2 * no) for code, p in res), "codes": _codes([code for code, _ in res])}
        recs.append(Record(f"pubkey_calc_{l}", "bee2hip_bignPubkeyCalcL_batch_dev", BIGN_SIZES if l == 128 else BIGN_WIDE_SIZES, calc_make,
                           lambda eng, T, c: eng.bignPubkeyCalcL_batch_dev(c.args["l"], T["privkeys"], T["pubkeys"], T["codes"]), calc_expect,
                           capture=257))

    T_LEN = 8
    for name, l, tmode in (("sign2_128_no_t", 128, None), ("sign2_128_shared_t", 128, "shared"), ("sign2_128_t_per_item", 128, "item"),
                           ("sign2_192_no_t", 192, None), ("sign2_256_t_per_item", 256, "item")):
        def make(orc, n, seed, l=l, tmode=tmode):
            no = l // 4
            bufs = [Buf("hashes", orc.fill(no * n, seed ^ 0x66)), Buf("privkeys", b"".join(privs(orc, l, n, seed)), 4)]
            if tmode:
                bufs.append(Buf("t", orc.fill(T_LEN * (n if tmode == "item" else 1), seed ^ 0x88), 4))
            bufs += [Buf("sigs", orc.fill(3 * l // 8 * n, seed ^ 0x55), 4, True), Buf("codes", orc.fill(4 * n, seed ^ 0x44), 4, True)]
            return Case(bufs, l=l, oid=E.LEVEL_OID[l], tmode=tmode)

        def call(eng, T, c):
            eng.bignSign2L_batch_dev(c.args["l"], c.args["oid"], T["hashes"], T["privkeys"], T["sigs"], T["codes"], t=T.get("t"),
                                     t_len=T_LEN if c.args["tmode"] else 0, t_shared=c.args["tmode"] != "item")

        def expect(orc, c):
            l, tmode = c.args["l"], c.args["tmode"]
            no, sg = l // 4, 3 * l // 8
            sigs, codes = [], []
            for i in range(len(c["hashes"]) // no):
                t = None if not tmode else c["t"][:T_LEN] if tmode == "shared" else c["t"][T_LEN * i:T_LEN * (i + 1)]
                code, sig = orc.sign2(l, c.args["oid"], c["hashes"][no * i:no * (i + 1)], c["privkeys"][no * i:no * (i + 1)], t)
                codes.append(code)
                sigs.append(sig if code == 0 else bytes(sg))
            return {"sigs": b"".join(sigs), "codes": _codes(codes)}
        recs.append(Record(name, "bee2hip_bignSign2L_batch_dev", BIGN_SIZES if l == 128 else BIGN_WIDE_SIZES, make, call, expect, capture=257))

    for l in (128, 192, 256):
        def k_make(orc, n, seed, l=l):
            no = l // 4
            return Case([Buf("hashes", orc.fill(no * n, seed ^ 0x66)), Buf("privkeys", b"".join(privs(orc, l, n, seed)), 4),
                         Buf("ks", b"".join(privs(orc, l, n, seed ^ 0x99)), 4),           # (one-time keys have the private keys' range)
                         Buf("sigs", orc.fill(3 * l // 8 * n, seed ^ 0x55), 4, True), Buf("codes", orc.fill(4 * n, seed ^ 0x44), 4, True)],
                        l=l, oid=E.LEVEL_OID[l])

        def k_expect(orc, c):
            l = c.args["l"]
            no, sg = l // 4, 3 * l // 8
            sigs, codes = [], []
            for i in range(len(c["hashes"]) // no):
                code, sig, _ = orc.sign_rnd(l, c.args["oid"], c["hashes"][no * i:no * (i + 1)], c["privkeys"][no * i:no * (i + 1)],
                                            c["ks"][no * i:no * (i + 1)])
                codes.append(code)
                sigs.append(sig if code == 0 else bytes(sg))
            return {"sigs": b"".join(sigs), "codes": _codes(codes)}
        recs.append(Record(f"signK_{l}", "bee2hip_bignSignKL_batch_dev", BIGN_SIZES if l == 128 else BIGN_WIDE_SIZES, k_make,
                           lambda eng, T, c: eng.bignSignKL_batch_dev(c.args["l"], c.args["oid"], T["hashes"], T["privkeys"], T["ks"], T["sigs"],
                                                                      T["codes"]), k_expect, capture=257))
    return recs


# ---- hashes: ragged batches, the fused bash + belt-MAC entry
RAGGED_LENS = (0, 1, 31, 32, 33, 4095, 4096, 4097)


def _hash_one(orc, alg, m):
    return orc.belt_hash(m) if alg == 0 else orc.bashHash(alg, m)[1]


def _ragged():
    recs = []
    for alg in (0, 128, 192, 256):
        for ordered in (False, True):
            if ordered and alg in (128, 192):
                continue

            def make(orc, n, seed, alg=alg, ordered=ordered):
                rng = np.random.default_rng(n)                                # (the lengths by the size alone: a replayed capture keeps its buffers)
                lens = rng.choice(RAGGED_LENS, size=n).astype(np.int64)       # message starts fall on every byte alignment
                offs = np.zeros(n + 1, dtype=np.int64)
                np.cumsum(lens, out=offs[1:])
                bufs = [Buf("data", orc.fill(int(offs[-1]), seed)), Buf("offsets", offs.tobytes(), 8)]
                if ordered:
                    bufs.append(Buf("order", np.argsort(-lens, kind="stable").astype(np.int32).tobytes(), 4))
                bufs.append(Buf("digests", orc.fill((alg // 4 if alg else 32) * n, seed ^ 0x44), 4, True))
                return Case(bufs, alg=alg, n=n)

            def call(eng, T, c):
                eng.hash_ragged_dev(c.args["alg"], T["data"], T["offsets"], T["digests"], c.args["n"], order=T.get("order"))

            def expect(orc, c):
                offs = np.frombuffer(c["offsets"], dtype=np.int64)
                return {"digests": b"".join(_hash_one(orc, c.args["alg"], c["data"][offs[i]:offs[i + 1]]) for i in range(c.args["n"]))}
            recs.append(Record(f"ragged_{'ordered_' if ordered else ''}{alg}",
                               "bee2hip_hash_ragged_ordered_dev" if ordered else "bee2hip_hash_ragged_dev", [200, 1500], make, call, expect,
                               capture=1500))
    return recs


def _fused():
    recs = []
    sizes = [(ml, n, off) for ml in (0, 16, 64, 100) for n in (1, 65, 1025) for off in (1, 4, 8)]
    for name, l, want in (("fused_hash_mac", 256, "hm"), ("fused_hash", 256, "h"), ("fused_mac", 256, "m"), ("fused_hash_mac_192", 192, "hm")):
        def make(orc, size, seed, l=l, want=want):
            ml, n, off = size
            # digests and tags are not checked by the entry: launch_bashHash_beltMAC takes the fused kernel when they are 8-byte
            # aligned (and msg_len is whole blocks) and the byte-wise per-message path otherwise
            bufs = [Buf("msgs", orc.fill(ml * n, seed))]
            if "h" in want:
                bufs.append(Buf("digests", orc.fill(l // 4 * n, seed ^ 0x44), off, True))
            if "m" in want:
                bufs.append(Buf("tags", orc.fill(8 * n, seed ^ 0x55), off, True))
            return Case(bufs, msg_len=ml, n=n, l=l)

        def call(eng, T, c):
            eng.bashHash_beltMAC_batch_dev(T["msgs"], c.args["msg_len"], c.args["l"], KEY, T.get("digests"), T.get("tags"), n=c.args["n"])

        def expect(orc, c, want=want):
            ml = c.args["msg_len"]
            msgs = [c["msgs"][i * ml:(i + 1) * ml] for i in range(c.args["n"])]
            out = {}
            if "h" in want:
                out["digests"] = b"".join(orc.bashHash(c.args["l"], m)[1] for m in msgs)
            if "m" in want:
                out["tags"] = b"".join(orc.mac(m, KEY) for m in msgs)
            return out
        recs.append(Record(name, "bee2hip_bashHash_beltMAC_batch_dev", sizes, make, call, expect, capture=(64, 1025, 8)))
    return recs


REGISTRY = (_bashF() + _belt_blocks() + _belt_sde() + _belt_cbc_batch() + _belt_dwp() + _bign_verify() + _bign_onekey_keyed()
            + _bign_keys_and_signing() + _ragged() + _fused())
BY_NAME = {r.name: r for r in REGISTRY}
assert len(BY_NAME) == len(REGISTRY)


def size_id(size):
    if isinstance(size, tuple):
        return "x".join("2p32m1" if s == (1 << 32) - 1 else str(s) for s in size)
    return str(size)


# ------------------------------------------------------------------------------------------------ placing a call in one allocation
class Layout:
    """every buffer of a case inside ONE allocation: [guard | pad | buffer | guard] per buffer, the buffer at off (16-aligned
    buffers) or at its own weakest alignment from a 256-byte boundary of the allocation"""

    def __init__(self, case, off16):
        self.at, pos = {}, 0
        for b in case.bufs:
            start = (pos + GUARD + 255) // 256 * 256 + (off16 if b.align == 16 else b.align)
            self.at[b.name] = (start, len(b.data))
            pos = start + len(b.data)
        self.total = (pos + GUARD + 255) // 256 * 256

    def image(self, case, pattern_seed, orc):
        """the allocation on entry: seeded pattern everywhere (a stray store of real output cannot look like it), the buffers' bytes
        in their places"""
        img = np.empty(self.total, dtype=np.uint8)
        orc.fill_np(img, pattern_seed)
        for b in case.bufs:
            s, n = self.at[b.name]
            img[s:s + n] = np.frombuffer(b.data, dtype=np.uint8)
        return img

    def expected(self, case, img, want):
        """(image after the call, mask of the bytes that are compared): everything but the outputs unchanged, the outputs the
        oracle's; all bytes are compared except the unsampled part of a sampled output"""
        exp, mask = img.copy(), np.ones(self.total, dtype=bool)
        outs = {b.name for b in case.bufs if b.out}
        assert set(want) == outs, (sorted(want), sorted(outs))
        for name, w in want.items():
            s, n = self.at[name]
            if isinstance(w, (bytes, bytearray)):
                assert len(w) == n, (name, len(w), n)
                w = [(0, w)]
            else:
                mask[s:s + n] = False
            for o, seg in w:
                assert o + len(seg) <= n
                exp[s + o:s + o + len(seg)] = np.frombuffer(seg, dtype=np.uint8)
                mask[s + o:s + o + len(seg)] = True
        return exp, mask

    def where(self, pos):
        """names the place of byte `pos` of the allocation for a failure message"""
        last = "guard in front of the first buffer"
        for name, (s, n) in sorted(self.at.items(), key=lambda kv: kv[1][0]):
            if pos < s:
                return f"{last} / guard in front of {name} ({s - pos} bytes before it)"
            if pos < s + n:
                return f"{name}[{pos - s}] of {n}"
            last = f"guard behind {name} ({pos - s - n} bytes after it)"
        return last
