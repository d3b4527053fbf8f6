"""A plain-Python model of the password-protected containers of STB 34.101.78 (src/crypto/bpki.c:206-548 of the reference:
bpkiPrivkeyWrap / Unwrap, bpkiShareWrap / Unwrap): the two DER frames with the reference's strictness (src/core/der.c), belt-pbkdf2
from tests/orc_belthmac.py and belt-kwp from tests/orc_beltkwp.py.  tests/test_bpki.py pins it to the reference's recorded outputs
(tests/golden/bpki.json); the GPU tests hold bee2hip_bpkiUnwrap_batch / bee2hip_bpkiWrap_batch to it."""
import functools

import orc_belthmac
import orc_beltkwp

ERR_OK, ERR_BAD_INPUT, ERR_NOT_IMPLEMENTED, ERR_BAD_FORMAT = 0, 109, 119, 306
ERR_BAD_SECKEY, ERR_BAD_PRIVKEY, ERR_BAD_SHAREKEY, ERR_BAD_KEYTOKEN = 503, 504, 508, 513
ITER_MAX, TOKEN_MAX = 1 << 17, 1024

OID = {"bign_pubkey": "1.2.112.0.2.0.34.101.45.2.1", "bels_share": "1.2.112.0.2.0.34.101.60.11",
       "pbes2": "1.2.840.113549.1.5.13", "pbkdf2": "1.2.840.113549.1.5.12", "belt_kwp256": "1.2.112.0.2.0.34.101.31.73",
       "hmac_hbelt": "1.2.112.0.2.0.34.101.47.12"}
PARAMS = ({24: "1.2.112.0.2.0.34.101.45.3.0", 32: "1.2.112.0.2.0.34.101.45.3.1", 48: "1.2.112.0.2.0.34.101.45.3.2",
           64: "1.2.112.0.2.0.34.101.45.3.3"},
          {17: "1.2.112.0.2.0.34.101.60.2.1", 25: "1.2.112.0.2.0.34.101.60.2.2", 33: "1.2.112.0.2.0.34.101.60.2.3"})
KEY_LENS = ((24, 32, 48, 64), (17, 25, 33))


# ---------------------------------------------------------------------------------------------------- writing
def der_len(n):
    if n < 128:
        return bytes([n])
    body = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([0x80 | len(body)]) + body


def tlv(tag, value):
    return bytes([tag]) + der_len(len(value)) + bytes(value)


def der_oid(text):
    arcs = [int(x) for x in text.split(".")]
    out = bytearray()
    for arc in [40 * arcs[0] + arcs[1]] + arcs[2:]:
        septets = [arc & 127]
        while arc >= 128:
            arc >>= 7
            septets.append(0x80 | (arc & 127))
        out += bytes(reversed(septets))
    return tlv(0x06, out)


def der_size(v):
    return tlv(0x02, v.to_bytes(v.bit_length() // 8 + 1, "big"))


def pki_build(kind, key):
    alg = tlv(0x30, der_oid(OID["bels_share" if kind else "bign_pubkey"]) + der_oid(PARAMS[kind][len(key)]))
    return tlv(0x30, der_size(0) + alg + tlv(0x04, key))


def epki_build(salt, iters, edata):
    prf = tlv(0x30, der_oid(OID["hmac_hbelt"]) + tlv(0x05, b""))
    kdf = tlv(0x30, der_oid(OID["pbkdf2"]) + tlv(0x30, tlv(0x04, salt) + der_size(iters) + prf))
    kwp = tlv(0x30, der_oid(OID["belt_kwp256"]) + tlv(0x05, b""))
    return tlv(0x30, tlv(0x30, der_oid(OID["pbes2"]) + tlv(0x30, kdf + kwp)) + tlv(0x04, edata))


# ---------------------------------------------------------------------------------------------------- reading
class Bad(Exception):
    pass


class Reader:
    """der.c's acceptance: one-octet tags, definite minimal lengths of at most 8 octets, values inside the buffer"""

    def __init__(self, data):
        self.d, self.pos = bytes(data), 0

    def tl(self, tag):
        d, p = self.d, self.pos
        if len(d) - p < 2 or d[p] != tag or d[p + 1] in (0x80, 0xFF):
            raise Bad
        n, used = d[p + 1], 2
        if n > 0x80:
            r = n - 0x80
            if r > 8 or len(d) - p - 2 < r or d[p + 2] == 0 or (r == 1 and d[p + 2] < 128):
                raise Bad
            n, used = int.from_bytes(d[p + 2:p + 2 + r], "big"), 2 + r
            if n == (1 << 64) - 1:
                raise Bad
        if n > len(d) - p - used:
            raise Bad
        self.pos += used
        return n

    def seq_start(self):
        n = self.tl(0x30)
        return self.pos + n

    def stop(self, end):
        if self.pos != end:
            raise Bad

    def null(self):
        if self.tl(0x05) != 0:
            raise Bad

    def oct(self):
        n = self.tl(0x04)
        v = self.d[self.pos:self.pos + n]
        self.pos += n
        return v

    def size(self):
        """derTSIZEDec; an INTEGER of no octets is 0 when the octet behind it has its top bit clear"""
        n = self.tl(0x02)
        if n > 9:
            raise Bad
        v = self.d[self.pos:self.pos + n]
        if n == 0:
            if self.pos >= len(self.d) or self.d[self.pos] & 0x80:
                raise Bad
            return 0
        if v[0] & 0x80 or (v[0] == 0 and n > 1 and not v[1] & 0x80) or (n == 9 and v[0] != 0):
            raise Bad
        self.pos += n
        return int.from_bytes(v, "big")

    def oid(self, text):
        """derOIDDec2: an arc is compared when it ends, so octets of an arc that never ends are not looked at"""
        want = [int(x) for x in text.split(".")]
        n = self.tl(0x06)
        val, got, first = 0, [], True
        for b in self.d[self.pos:self.pos + n]:
            if val & 0xFE000000 or (val == 0 and b == 0x80):
                raise Bad
            val = (val << 7 | (b & 127)) & 0xFFFFFFFF
            if b & 0x80:
                continue
            if first:
                d1 = 0 if val < 40 else 1 if val < 80 else 2
                val -= 40 * d1
                got.append(d1)
                first = False
            got.append(val)
            if got != want[:len(got)]:
                raise Bad
            val = 0
        if got != want:
            raise Bad
        self.pos += n


def epki_parse(epki):
    """-> (salt, iter, offset of encData, its length) or None"""
    try:
        d = Reader(epki)
        e_epki = d.seq_start()
        e_alg = d.seq_start()
        d.oid(OID["pbes2"])
        e_pbes2 = d.seq_start()
        e_kdf = d.seq_start()
        d.oid(OID["pbkdf2"])
        e_par = d.seq_start()
        salt = d.oct()
        if len(salt) != 8:
            raise Bad
        iters = d.size()
        e_prf = d.seq_start()
        d.oid(OID["hmac_hbelt"])
        d.null()
        d.stop(e_prf)
        d.stop(e_par)
        d.stop(e_kdf)
        e_kwp = d.seq_start()
        d.oid(OID["belt_kwp256"])
        d.null()
        d.stop(e_kwp)
        d.stop(e_pbes2)
        d.stop(e_alg)
        edata = d.oct()
        d.stop(e_epki)
        d.stop(len(d.d))
        return salt, iters, d.pos - len(edata), len(edata)
    except Bad:
        return None


def pki_parse(kind, pki):
    """-> the key or None"""
    try:
        d = Reader(pki)
        e_pki = d.seq_start()
        if d.size() != 0:
            raise Bad
        e_alg = d.seq_start()
        d.oid(OID["bels_share" if kind else "bign_pubkey"])
        mark, want = d.pos, None
        for n, text in PARAMS[kind].items():
            try:
                d.pos = mark
                d.oid(text)
                want = n
                break
            except Bad:
                pass
        if want is None:
            raise Bad
        d.stop(e_alg)
        key = d.oct()
        if len(key) != want:
            raise Bad
        d.stop(e_pki)
        d.stop(len(d.d))
        return key
    except Bad:
        return None


# ---------------------------------------------------------------------------------------------------- the containers
@functools.lru_cache(maxsize=None)
def kek(pwd, iters, salt):
    return orc_belthmac.pbkdf2(pwd, iters, salt)


def unwrap(kind, epki, pwd, limits=True):
    """-> (code, key): bee2's code in bee2's order; with limits, the two refusals of the batch (ERR_NOT_IMPLEMENTED)"""
    e = epki_parse(epki)
    if e is None:
        return ERR_BAD_FORMAT, b""
    salt, iters, off, n = e
    if iters == 0:
        return ERR_BAD_INPUT, b""
    if limits and iters > ITER_MAX:
        return ERR_NOT_IMPLEMENTED, b""
    if n < 32:
        return ERR_BAD_INPUT, b""
    if limits and n > TOKEN_MAX:
        return ERR_NOT_IMPLEMENTED, b""
    code, pki = orc_beltkwp.unwrap(epki[off:off + n], None, kek(bytes(pwd), iters, bytes(salt)))
    if code:
        return code, b""
    key = pki_parse(kind, pki)
    if key is None:
        return ERR_BAD_FORMAT, b""
    if kind == 1 and not 1 <= key[0] <= 16:
        return ERR_BAD_SHAREKEY, b""
    return ERR_OK, key


def wrap(kind, key, pwd, salt, iters):
    """-> (code, container)"""
    if iters < 10000:
        return ERR_BAD_INPUT, b""
    if len(key) not in KEY_LENS[kind] or (kind == 1 and not 1 <= key[0] <= 16):
        return (ERR_BAD_SECKEY if kind else ERR_BAD_PRIVKEY), b""
    return ERR_OK, epki_build(salt, iters, seal(kind, key, pwd, salt, iters))


def seal(kind, key, pwd, salt, iters, pki=None):
    """the token of a key's frame (or of any `pki`) under the password's key: no limits on iters"""
    return orc_beltkwp.wrap(pki_build(kind, key) if pki is None else pki, None, kek(bytes(pwd), iters, bytes(salt)))
