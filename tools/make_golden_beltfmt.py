"""tests/golden/belt_fmt.json: belt-fmt rows with the reference's own outputs and block counts (oracle/_ref/libbee2ref.so:
beltFMTEncr / beltFMTDecr / beltFMT_keep, src/crypto/belt/belt_fmt.c).  Build container only.

  * "rows": tests/beltfmtgrid.py fixture_cases() -- every shape x key lengths 16 / 24 / 32 x both directions, some without iv,
    some with symbols at or above the modulus, then the seam shapes of the launch plan (PLAN_SHAPES) with one key length each;
    inputs come from each row's seed, outputs as hex (sha256 above 64 symbols), with the block counts b1 / b2 the reference
    uses for the two halves;
  * "blocks": [mod, n, b] for beltfmtgrid.block_pairs(), read off beltFMT_keep (its state ends in 8 (b(mod, n1) + 1) octets).
The script decrypts every encrypted in-range row with the reference again and stops on a difference."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import refgen  # noqa: E402
import beltfmtgrid as G  # noqa: E402

L = refgen.ref()
_sz = ctypes.c_size_t
L.beltFMT_keep.restype = _sz


def ref_crypt(decr, mod, syms, key, iv):
    n = len(syms)
    src, dst = (ctypes.c_uint16 * n)(*syms), (ctypes.c_uint16 * n)()
    code = (L.beltFMTDecr if decr else L.beltFMTEncr)(dst, ctypes.c_uint32(mod), src, _sz(n), key, _sz(len(key)), iv)
    assert code == 0, code
    return list(dst)


def keep(mod, count):
    return L.beltFMT_keep(ctypes.c_uint32(mod), _sz(count))


BASE = keep(65536, 2) - 16                     # b(65536, 1) = 1


def ref_blocks(mod, n):
    """b(mod, n) as the reference computes it: n is the left half of a record of max(2, 2 n - 1) symbols"""
    return (keep(mod, max(2, 2 * n - 1)) - BASE) // 8 - 1


def main():
    rows = G.fixture_cases()
    for c in rows:
        x = G.case_inputs(c)
        out = ref_crypt(c["decr"], c["mod"], x["symbols"], x["key"], x["iv"])
        if not c["oor"]:
            assert ref_crypt(1 - c["decr"], c["mod"], out, x["key"], x["iv"]) == x["symbols"]
        c.update(out=G.encode(out), b1=ref_blocks(c["mod"], (c["count"] + 1) // 2), b2=ref_blocks(c["mod"], c["count"] // 2))
    blocks = [[m, n, ref_blocks(m, n)] for m, n in G.block_pairs()]
    path = os.path.join(ROOT, "tests", "golden", "belt_fmt.json")
    with open(path, "w") as f:
        json.dump({"rows": rows, "blocks": blocks}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes;", len(rows), "rows;", len(blocks), "block counts")


if __name__ == "__main__":
    main()
