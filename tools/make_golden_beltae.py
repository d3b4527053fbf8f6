"""tests/golden/belt_ae_ragged.json: belt-dwp / belt-che records with the reference's own ciphertext and tag
(oracle/_ref/libbee2ref.so: beltDWPWrap / beltCHEWrap, src/crypto/belt/belt_dwp.c, belt_che.c).  Build container only.

  * "records": tests/beltaegrid.py fixture_cases() -- both modes x key lengths 16 / 24 / 32 x every text length of the GPU
    grid, header lengths cycling through the grid's; inputs come from each record's seed, outputs as hex;
  * "carry": the iv of the carry record (beltaegrid.CARRY_KEY, 2^12 + 16 blocks): the first iv of a counter pattern with
    E_K(iv) mod 2^32 >= 2^32 - 2^12, so the belt-dwp counter carries out of its low 32-bit word inside the record; its tag
    and the SHA-256 of its ciphertext (65 792 octets are not worth committing).
The script unwraps every record with the reference again and stops on a difference."""
import ctypes
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import refgen  # noqa: E402
import beltaegrid as G  # noqa: E402

L = refgen.ref()
_sz = ctypes.c_size_t


def ref_wrap(mode, key, iv, hdr, text):
    name = G.MODES[mode]
    dest, mac = ctypes.create_string_buffer(max(len(text), 1)), ctypes.create_string_buffer(8)
    code = getattr(L, f"belt{name}Wrap")(dest, mac, bytes(text), _sz(len(text)), bytes(hdr), _sz(len(hdr)), bytes(key),
                                         _sz(len(key)), bytes(iv))
    assert code == 0, code
    ct = dest.raw[:len(text)]
    back = ctypes.create_string_buffer(max(len(text), 1))
    code = getattr(L, f"belt{name}Unwrap")(back, ct, _sz(len(ct)), bytes(hdr), _sz(len(hdr)), mac.raw, bytes(key), _sz(len(key)),
                                           bytes(iv))
    assert code == 0 and back.raw[:len(text)] == bytes(text)
    return ct, mac.raw


def find_carry_iv(trials=1 << 22):
    """the first iv = counter (64-bit little-endian) || zeros whose E_K(iv) has a low word of at least 2^32 - 2^12"""
    step = 1 << 16
    for base in range(0, trials, step):
        ivs = b"".join(struct.pack("<QQ", c, 0) for c in range(base, base + step))
        out = ctypes.create_string_buffer(len(ivs))
        assert L.beltECBEncr(out, ivs, _sz(len(ivs)), G.CARRY_KEY, _sz(len(G.CARRY_KEY))) == 0
        for k in range(step):
            if struct.unpack_from("<I", out.raw, 16 * k)[0] >= (1 << 32) - (1 << 12):
                return ivs[16 * k:16 * k + 16]
    raise RuntimeError("no carry iv found")


def main():
    records = G.fixture_cases()
    for c in records:
        x = G.case_inputs(c)
        ct, tag = ref_wrap(c["mode"], x["key"], x["iv"], x["hdr"], x["text"])
        c.update(ct=ct.hex(), tag=tag.hex())
    iv = find_carry_iv()
    x = G.carry_inputs(iv.hex())
    ct, tag = ref_wrap(0, x["key"], x["iv"], x["hdr"], x["text"])
    carry = {"iv": iv.hex(), "tag": tag.hex(), "ct_sha256": G.sha(ct)}
    path = os.path.join(ROOT, "tests", "golden", "belt_ae_ragged.json")
    with open(path, "w") as f:
        json.dump({"records": records, "carry": carry}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes;", len(records), "records; carry iv", iv.hex())


if __name__ == "__main__":
    main()
