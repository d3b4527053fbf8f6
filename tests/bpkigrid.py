"""Rows of tests/golden/bpki.json (tools/make_golden_bpki.py records the reference's outputs for them) and the builders of its
malformed corpus: the EncryptedPrivateKeyInfo / PrivateKeyInfo frames of src/crypto/bpki.c with one fault each.  No GPU and no
reference here; a row's inputs come from its seed."""
import random

import orc_bpki as M

PWD_LENS = (0, 1, 32, 33, 100)                 # (a password over 32 octets is hashed first)


def good_cases():
    """both kinds at every key length x every password length at 10000 iterations; at 65536 (a SIZE of 3 octets: the frame
    is one octet longer) one key length a kind x the shortest and the longest password"""
    out = []
    for kind in (0, 1):
        for j, key_len in enumerate(M.KEY_LENS[kind]):
            for k, pwd_len in enumerate(PWD_LENS):
                out.append({"kind": kind, "key_len": key_len, "iter": 10000, "pwd_len": pwd_len, "seed": 7100000 + 1000 * kind + 10 * j + k})
        for k, pwd_len in enumerate((0, 100)):
            out.append({"kind": kind, "key_len": M.KEY_LENS[kind][1], "iter": 65536, "pwd_len": pwd_len, "seed": 7200000 + 1000 * kind + k})
    return out


def case_inputs(c):
    rnd = random.Random(c["seed"])
    key = bytearray(rnd.randbytes(c["key_len"]))
    if c["kind"] == 1:
        key[0] = 1 + rnd.randrange(16)
    x = {"key": bytes(key), "pwd": rnd.randbytes(c["pwd_len"]), "salt": rnd.randbytes(8)}
    wrong = bytearray(x["pwd"] or b"\0")
    wrong[rnd.randrange(len(wrong))] ^= 1 << rnd.randrange(8)
    x["wrong_pwd"] = bytes(wrong)
    return x


def base_case(kind, rows=None):
    """the good row (of `rows`: the fixture's) the malformed corpus of a kind is derived from: 32 / 25 octets, 10000 iterations,
    a 32-octet password"""
    return next(c for c in (good_cases() if rows is None else rows) if c["kind"] == kind and c["key_len"] == M.KEY_LENS[kind][1] and c["iter"] == 10000
                and c["pwd_len"] == 32)


# ---------------------------------------------------------------------------------------------------- frames with one fault
def _nonminimal(n):
    if n < 128:
        return bytes([0x81, n])
    body = n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([0x80 | (len(body) + 1), 0]) + body


def _node(faults, name, tag, value):
    f = faults.get(name)
    if f == "nonminimal":
        return bytes([tag]) + _nonminimal(len(value)) + value
    if f == "indefinite":
        return bytes([tag, 0x80]) + value + b"\0\0"
    return M.tlv(tag, value)


def _oid(faults, name, text):
    v = bytearray(M.der_oid(text)[2:])
    f = faults.get(name)
    if f == "flip":                              # (bit 4: the last arc becomes one that no OID of either frame has)
        v[-1] ^= 0x10
    elif f == "open":                            # an arc that never ends behind the last one
        v += b"\x81"
    elif f == "zero":                            # 0x80 in front of the last arc
        v[-1:] = bytes([0x80, v[-1]])
    return M.tlv(0x06, v)


def epki_frame(salt, iters, edata, **faults):
    """the outer frame; faults: node -> 'nonminimal' / 'indefinite' (epki, alg, pbes2, kdf, par, prf, kwp, salt_oct, edata_oct),
    OID -> 'flip' / 'open' / 'zero' (oid_pbes2, oid_pbkdf2, oid_hmac, oid_kwp), iter_der -> the INTEGER's octets as given"""
    size = faults.get("iter_der", None)
    size = M.der_size(iters) if size is None else size
    prf = _node(faults, "prf", 0x30, _oid(faults, "oid_hmac", M.OID["hmac_hbelt"]) + M.tlv(0x05, b""))
    par = _node(faults, "par", 0x30, _node(faults, "salt_oct", 0x04, salt) + size + prf)
    kdf = _node(faults, "kdf", 0x30, _oid(faults, "oid_pbkdf2", M.OID["pbkdf2"]) + par)
    kwp = _node(faults, "kwp", 0x30, _oid(faults, "oid_kwp", M.OID["belt_kwp256"]) + M.tlv(0x05, b""))
    pbes2 = _node(faults, "pbes2", 0x30, kdf + kwp)
    alg = _node(faults, "alg", 0x30, _oid(faults, "oid_pbes2", M.OID["pbes2"]) + pbes2)
    return _node(faults, "epki", 0x30, alg + _node(faults, "edata_oct", 0x04, edata))


def pki_frame(kind, key, **faults):
    """the inner frame; faults: version -> its INTEGER's octets, params -> another OID, oid_alg / oid_params -> 'flip', pki / algid /
    key_oct -> 'nonminimal', tail -> octets behind the frame"""
    alg = _node(faults, "algid", 0x30, _oid(faults, "oid_alg", M.OID["bels_share" if kind else "bign_pubkey"])
                + _oid(faults, "oid_params", faults.get("params", M.PARAMS[kind].get(len(key), M.PARAMS[kind][M.KEY_LENS[kind][1]]))))
    return _node(faults, "pki", 0x30, faults.get("version", M.der_size(0)) + alg + _node(faults, "key_oct", 0x04, key)) + faults.get("tail", b"")


def outer_variants(salt, iters, edata):
    """[(name, container)]: every outer fault but the truncations, which are cuts of the good container"""
    good = epki_frame(salt, iters, edata)
    assert good == M.epki_build(salt, iters, edata)
    out = [("trailing_octet", good + b"\0")]
    for name in ("oid_pbes2", "oid_pbkdf2", "oid_hmac", "oid_kwp"):
        out += [(f"{name}_{f}", epki_frame(salt, iters, edata, **{name: f})) for f in ("flip", "open", "zero")]
    for name in ("epki", "alg", "pbes2", "kdf", "par", "prf", "kwp", "salt_oct", "edata_oct"):
        out.append((f"{name}_nonminimal", epki_frame(salt, iters, edata, **{name: "nonminimal"})))
    out.append(("epki_indefinite", epki_frame(salt, iters, edata, epki="indefinite")))
    out.append(("prf_indefinite", epki_frame(salt, iters, edata, prf="indefinite")))
    out.append(("iter_zero", epki_frame(salt, iters, edata, iter_der=M.der_size(0))))
    out.append(("iter_no_octets", epki_frame(salt, iters, edata, iter_der=b"\x02\x00")))
    out.append(("iter_negative", epki_frame(salt, iters, edata, iter_der=b"\x02\x02\xA7\x10")))
    out.append(("iter_zero_in_front", epki_frame(salt, iters, edata, iter_der=b"\x02\x03\x00\x27\x10")))
    out.append(("iter_9_octets", epki_frame(salt, iters, edata, iter_der=b"\x02\x09\x01" + bytes(8))))
    out.append(("iter_10_octets", epki_frame(salt, iters, edata, iter_der=b"\x02\x0A\x00\x80" + bytes(8))))
    out.append(("salt_7", epki_frame(salt[:7], iters, edata)))
    out.append(("salt_9", epki_frame(salt + b"\0", iters, edata)))
    out.append(("edata_31", epki_frame(salt, iters, edata[:31])))
    out.append(("edata_32", epki_frame(salt, iters, edata[:32])))
    out.append(("edata_0", epki_frame(salt, iters, b"")))
    out.append(("null_as_empty_octets", good.replace(b"\x05\x00", b"\x04\x00", 1)))
    out.append(("wrong_outer_tag", b"\x31" + good[1:]))
    out.append(("long_tag", b"\x3f" + good[1:]))
    return out


def inner_variants(kind, key):
    """[(name, inner frame)]: frames that belt-kwp accepts once re-sealed and bpkiPrivkeyDec / bpkiShareDec must refuse --
    but for the last two of a share, whose frame is fine and whose first octet is not"""
    other = M.PARAMS[1 - kind][M.KEY_LENS[1 - kind][0]]
    next_len = M.PARAMS[kind][M.KEY_LENS[kind][2]]
    out = [("inner_version_1", pki_frame(kind, key, version=M.der_size(1))),
           ("inner_version_no_octets", pki_frame(kind, key, version=b"\x02\x00")),
           ("inner_params_of_other_kind", pki_frame(kind, key, params=other)),
           ("inner_params_of_next_length", pki_frame(kind, key, params=next_len)),
           ("inner_params_flip", pki_frame(kind, key, oid_params="flip")),
           ("inner_alg_flip", pki_frame(kind, key, oid_alg="flip")),
           ("inner_key_short", pki_frame(kind, key[:-1], params=M.PARAMS[kind][len(key)])),
           ("inner_key_long", pki_frame(kind, key + b"\1", params=M.PARAMS[kind][len(key)])),
           ("inner_trailing_octet", pki_frame(kind, key, tail=b"\0")),
           ("inner_pki_nonminimal", pki_frame(kind, key, pki="nonminimal")),
           ("inner_algid_nonminimal", pki_frame(kind, key, algid="nonminimal")),
           ("inner_key_nonminimal", pki_frame(kind, key, key_oct="nonminimal"))]
    if kind == 1:
        out += [("inner_share_first_octet_0", pki_frame(kind, b"\0" + key[1:])), ("inner_share_first_octet_17", pki_frame(kind, b"\x11" + key[1:]))]
    return out
