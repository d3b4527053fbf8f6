"""tests/golden/belt_kwp.json: belt-kwp rows with the reference's own outputs (oracle/_ref/libbee2ref.so: beltKWPWrap /
beltKWPUnwrap, src/crypto/belt/belt_kwp.c).  Build container only.

  * "rows": tests/beltkwpgrid.py fixture_cases() -- wrap counts 16..99, 127, 128, 129, 1007, 1008, 288, 289, 592, 593 x key lengths 16 / 24 / 32 x
    with and without header; inputs come from each row's seed.  Per row: the token; code and output of unwrapping the token
    with one bit flipped; code and output of unwrapping the token under a wrong header.  Outputs as hex (sha256 above 64
    octets).
  * "a21", "a22": the standard's vectors A.21 and A.22 (test/crypto/belt_test.c:565-592) as the reference computes them.
The script unwraps every token with the reference again and stops on a difference."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import refgen  # noqa: E402
import beltkwpgrid as G  # noqa: E402

L = refgen.ref()
_sz = ctypes.c_size_t
L.beltWBL_keep.restype = _sz                    # belt.h: beltKWP_keep / Start / StepD are names for the beltWBL ones


def ref_wrap(src, header, key):
    dst = ctypes.create_string_buffer(len(src) + 16)
    code = L.beltKWPWrap(dst, bytes(src), _sz(len(src)), header, bytes(key), _sz(len(key)))
    assert code == 0, code
    return dst.raw


def ref_unwrap(token, header, key):
    dst = ctypes.create_string_buffer(b"\xAA" * (len(token) - 16), len(token) - 16)
    code = L.beltKWPUnwrap(dst, bytes(token), _sz(len(token)), header, bytes(key), _sz(len(key)))
    return code, dst.raw


def main():
    rows = G.fixture_cases()
    for c in rows:
        x = G.case_inputs(c)
        token = ref_wrap(x["src"], x["header"], x["key"])
        assert ref_unwrap(token, x["header"], x["key"]) == (0, x["src"])
        fc, fo = ref_unwrap(G.flipped(token, x["flip"]), x["header"], x["key"])
        hc, ho = ref_unwrap(token, x["wrong_header"], x["key"])
        c.update(token=G.encode(token), flip_code=fc, flip_out=G.encode(fo), hdr_code=hc, hdr_out=G.encode(ho))
    H = refgen.beltH()
    a21 = ref_wrap(H[:32], H[32:48], H[128:160])
    assert a21.hex().upper().startswith("49A38EE1") and a21.hex().upper().endswith("1DC9F6C8")
    # A.22: belt-wbl decryption of beltH()[64..112) under beltH()[160..192) gives key || header; the one-shot then accepts it
    st = ctypes.create_string_buffer(L.beltWBL_keep())
    buf = ctypes.create_string_buffer(H[64:112], 48)
    L.beltWBLStart(st, H[160:192], _sz(32))
    L.beltWBLStepD(buf, _sz(48), st)
    code, key22 = ref_unwrap(H[64:112], buf.raw[32:], H[160:192])
    assert code == 0 and key22 == buf.raw[:32] and key22.hex().upper().startswith("92632EE0")
    path = os.path.join(ROOT, "tests", "golden", "belt_kwp.json")
    with open(path, "w") as f:
        json.dump({"rows": rows, "a21": {"token": a21.hex()}, "a22": {"key": key22.hex(), "header": buf.raw[32:].hex()}}, f, indent=0,
                  sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes;", len(rows), "rows")


if __name__ == "__main__":
    main()
