"""belt-hmac and belt-pbkdf2 (STB 34.101.31; src/crypto/belt/belt_hmac.c, belt_pbkdf.c) as compositions of the oracle's
belt-hash: the model the batched kernel, its CPU shim and the host path are held to.  tests/golden/belt_hmac.json pins it to the
reference's own outputs."""
import functools

import orclib

ERR_OK, ERR_BAD_INPUT, ERR_NOT_IMPLEMENTED, ERR_BAD_MAC = 0, 109, 119, 511


@functools.lru_cache(maxsize=None)
def _orc():
    return orclib.load()


def belt_hash(msg):
    return _orc().belt_hash(bytes(msg))


def _pads(key):
    key = bytes(key)
    if len(key) > 32:
        key = belt_hash(key)
    key = key.ljust(32, b"\0")
    return bytes(b ^ 0x36 for b in key), bytes(b ^ 0x5C for b in key)


def hmac(key, msg):
    ipad, opad = _pads(key)
    return belt_hash(opad + belt_hash(ipad + bytes(msg)))


def pbkdf2(pwd, iters, salt):
    assert iters >= 1
    ipad, opad = _pads(pwd)
    t = belt_hash(opad + belt_hash(ipad + bytes(salt) + b"\0\0\0\1"))
    acc = int.from_bytes(t, "little")
    for _ in range(iters - 1):
        t = belt_hash(opad + belt_hash(ipad + t))
        acc ^= int.from_bytes(t, "little")
    return acc.to_bytes(32, "little")


def verify(key, msg, mac):
    """the code of a record whose first len(mac) octets are compared"""
    return ERR_OK if hmac(key, msg)[:len(mac)] == bytes(mac) else ERR_BAD_MAC
