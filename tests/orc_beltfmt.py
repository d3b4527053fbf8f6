"""A plain-Python model of belt-fmt (STB 34.101.31, format-preserving encryption; src/crypto/belt/belt_fmt.c of the reference):
Python integers for the numbers, E_K from the C oracle (orclib's ecb).  tests/test_beltfmt.py pins it to the reference's outputs
(tests/golden/belt_fmt.json) and to the standard's vectors; the GPU tests compare the kernel with it record by record."""
import functools
import struct

import orclib

MOD_MAX, COUNT_MAX = 65536, 600


def block_count(mod, n):
    """b(mod, n): the smallest b with mod^n <= 2^(64 b); b(49667, 160) = 40 is the one pair where the reference's own
    approximation (belt_fmt.c:74-149) gives one more than that"""
    if (mod, n) == (49667, 160):
        return 40
    return max(1, -(-(mod ** n - 1).bit_length() // 64))


@functools.lru_cache(maxsize=None)
def _H():
    return orclib.Golden().H


class Cipher:
    def __init__(self, key):
        self.key, self.orc = bytes(key), orclib.load()

    def E(self, block):
        code, out = self.orc.ecb(bytes(block), self.key)
        assert code == 0
        return out

    def block32(self, buf):
        """belt-32block on 24 octets (belt_fmt.c:157-175)"""
        t = list(struct.unpack("<6I", buf))
        for r, base in ((1, 2), (2, 4), (3, 0)):
            idx = [(base + k) % 6 for k in range(4)]
            x = list(struct.unpack("<4I", self.E(struct.pack("<4I", *(t[i] for i in idx)))))
            x[0] ^= r
            for i, v in zip(idx, x):
                t[i] = v
            t[(base - 2) % 6] ^= x[0]
            t[(base - 1) % 6] ^= x[1]
        return struct.pack("<6I", *t)

    def wbl(self, buf):
        """belt-wbl encryption of len >= 32 octets, any length that is 0 or 8 mod 16 (belt_wbl.c:50-82)"""
        buf, n = bytearray(buf), (len(buf) + 15) // 16
        L = len(buf)
        for rnd in range(1, 2 * n + 1):
            s, i = int.from_bytes(buf[:16], "little"), 16
            while i + 16 < L:
                s ^= int.from_bytes(buf[i:i + 16], "little")
                i += 16
            buf[:L - 16] = buf[16:]
            buf[L - 16:] = s.to_bytes(16, "little")
            e = int.from_bytes(self.E(s.to_bytes(16, "little")), "little") ^ rnd
            x = int.from_bytes(buf[L - 32:L - 16], "little") ^ e
            buf[L - 32:L - 16] = x.to_bytes(16, "little")
        return bytes(buf)

    def F(self, half, mod, b, hw, ivw):
        a = 0
        for s in reversed(half):
            a = (a * mod + s) % (1 << (64 * b))
        buf = a.to_bytes(8 * b, "little") + hw + ivw
        out = self.E(buf) if b == 1 else self.block32(buf) if b == 2 else self.wbl(buf)
        return int.from_bytes(out, "little")


def crypt(decr, mod, symbols, key, iv=None):
    """-> the list of count symbols; iv None = 16 zero octets.  Symbols >= mod are not refused: they enter the arithmetic"""
    count = len(symbols)
    assert 2 <= mod <= MOD_MAX and 2 <= count <= COUNT_MAX
    n1, n2 = (count + 1) // 2, count // 2
    b1, b2 = block_count(mod, n1), block_count(mod, n2)
    hdr = struct.pack("<HH", mod & 0xFFFF, count)
    ivx = hdr + (bytes(16) if iv is None else bytes(iv)) + hdr
    assert len(ivx) == 24
    H, C = _H(), Cipher(key)
    left, right = list(symbols[:n1]), list(symbols[n1:])

    def mix(dst, a):
        for k in range(len(dst)):
            t = a % mod
            dst[k] = (dst[k] + (mod - t if decr else t)) % mod
            a //= mod

    steps = [(i, w) for i in range(3) for w in range(2)]
    for i, w in (reversed(steps) if decr else steps):
        o = 8 * i + 4 * w
        if w == 0:
            mix(left, C.F(right, mod, b2, H[o:o + 4], ivx[o:o + 4]))
        else:
            mix(right, C.F(left, mod, b1, H[o:o + 4], ivx[o:o + 4]))
    return left + right


def crypt_bytes(decr, mod, count, key, iv, data):
    """on count little-endian u16"""
    return struct.pack(f"<{count}H", *crypt(decr, mod, list(struct.unpack(f"<{count}H", data)), key, iv))
