"""A plain-Python model of belt-kwp (STB 34.101.31, key wrap; src/crypto/belt/belt_kwp.c of the reference): belt-wbl in its
byte-level shifting form (belt_wbl.c:50-82 and :129-159) over key || header, E_K from the C oracle (orclib's ecb).
tests/test_beltkwp.py pins it to the reference's outputs (tests/golden/belt_kwp.json) and to the standard's vectors; the GPU
tests compare the kernel with it record by record."""
import orclib

ERR_OK, ERR_BAD_KEYTOKEN = 0, 513
TOKEN_MAX = 1024


class Cipher:
    def __init__(self, key):
        self.key, self.orc = bytes(key), orclib.load()

    def E(self, block):
        code, out = self.orc.ecb(bytes(block), self.key)
        assert code == 0
        return out


def _xor(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


def _sum(buf, first, L):
    """the XOR of the blocks at octets first, first + 16 .. while offset + 16 < L (integers: the tests call this often)"""
    acc = 0
    for i in range(first, L - 16, 16):
        acc ^= int.from_bytes(buf[i:i + 16], "little")
    return acc.to_bytes(16, "little")


def wbl_encr(buf, key):
    """belt-wbl encryption of len >= 32 octets, any length"""
    C, buf, L = Cipher(key), bytearray(buf), len(buf)
    assert L >= 32
    for rnd in range(1, 2 * ((L + 15) // 16) + 1):
        s = _sum(buf, 0, L)
        buf[:L - 16] = buf[16:]
        buf[L - 16:] = s
        e = _xor(C.E(s), rnd.to_bytes(16, "little"))
        buf[L - 32:L - 16] = _xor(buf[L - 32:L - 16], e)
    return bytes(buf)


def wbl_decr(buf, key):
    C, buf, L = Cipher(key), bytearray(buf), len(buf)
    assert L >= 32
    for rnd in range(2 * ((L + 15) // 16), 0, -1):
        s = bytes(buf[L - 16:])
        buf[16:] = buf[:L - 16]
        buf[:16] = s
        e = _xor(C.E(s), rnd.to_bytes(16, "little"))
        buf[L - 16:] = _xor(buf[L - 16:], e)
        buf[:16] = _xor(buf[:16], _sum(buf, 16, L))
    return bytes(buf)


def wrap(src, header, key):
    """beltKWPWrap -> the token of len(src) + 16 octets; header None = 16 zero octets"""
    assert len(src) >= 16 and len(key) in (16, 24, 32)
    return wbl_encr(bytes(src) + (bytes(16) if header is None else bytes(header)), key)


def unwrap(token, header, key):
    """beltKWPUnwrap -> (code, len(token) - 16 octets: the key, or zeros when the token is refused)"""
    assert len(token) >= 32 and len(key) in (16, 24, 32)
    out = wbl_decr(token, key)
    if out[-16:] != (bytes(16) if header is None else bytes(header)):
        return ERR_BAD_KEYTOKEN, bytes(len(token) - 16)
    return ERR_OK, out[:-16]
