"""tests/golden/belt_hmac.json: belt-hmac / belt-pbkdf2 rows with the reference's own outputs (oracle/_ref/libbee2ref.so:
beltHMAC, beltPBKDF2; src/crypto/belt/belt_hmac.c, belt_pbkdf.c).  Build container only.

  * "rows": tests/belthmacgrid.py fixture_cases() -- key / password lengths x message / salt lengths, beltHMAC once and
    beltPBKDF2 at 1, 2, 3 and 50 iterations; inputs come from each row's seed, the output is hex.
  * "b1": the three HMAC vectors of the standard (test/crypto/belt_test.c:787-819): keys of 29, 32 and 42 octets.
  * "pbkdf2": the PBKDF2 vectors of test/crypto/bign_test.c:521-553 (E.5 and the two checked against OpenSSL)."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import refgen  # noqa: E402
import belthmacgrid as G  # noqa: E402

L = refgen.ref()
_sz = ctypes.c_size_t


def ref_hmac(key, msg):
    out = ctypes.create_string_buffer(32)
    assert L.beltHMAC(out, bytes(msg), _sz(len(msg)), bytes(key), _sz(len(key))) == 0
    return out.raw


def ref_pbkdf2(pwd, iters, salt):
    out = ctypes.create_string_buffer(32)
    assert L.beltPBKDF2(out, bytes(pwd), _sz(len(pwd)), _sz(iters), bytes(salt), _sz(len(salt))) == 0
    return out.raw


def main():
    rows = G.fixture_cases()
    for c in rows:
        key, msg = G.case_inputs(c)
        c["out"] = (ref_hmac(key, msg) if c["kind"] == "hmac" else ref_pbkdf2(key, c["iter"], msg)).hex()
    H = refgen.beltH()
    b1 = [{"key_len": k, "mac": ref_hmac(H[128:128 + k], H[192:224]).hex()} for k in (29, 32, 42)]
    assert b1[0]["mac"].upper().startswith("D4828E63") and b1[0]["mac"].upper().endswith("E930676B")
    vec = [(b"B194BAC80A08F53B", 10000, H[192:200]), (b"zed", 2048, bytes.fromhex("49FEFF8076CD9480")),
           (b"zed", 10000, bytes.fromhex("C65017E4F108BCF0"))]
    pb = [{"pwd": p.decode(), "iter": it, "salt": s.hex(), "key": ref_pbkdf2(p, it, s).hex()} for p, it, s in vec]
    assert pb[0]["key"].upper().startswith("3D331BBB") and pb[1]["key"].upper().startswith("7249B478")
    assert pb[2]["key"].upper().startswith("E4832925")
    path = os.path.join(ROOT, "tests", "golden", "belt_hmac.json")
    with open(path, "w") as f:
        json.dump({"rows": rows, "b1": b1, "pbkdf2": pb}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes;", len(rows), "rows")


if __name__ == "__main__":
    main()
