"""tests/golden/bash_prg.json: bash-prg known answers, every output taken from the reference itself
(oracle/_ref/libbee2ref.so, src/crypto/bash/bash_prg.c).  Build container only.

  * "vectors": STB 34.101.77 A.5.1 - A.5.7 (prg-hash) and A.6 (prg-ae) with the inputs of test/crypto/bash_test.c (octets of
    the belt S-box table), inputs and outputs as hex;
  * "random": about 200 cases over all six (l, d) (tests/orc_bashprg.py random_cases): seeds and lengths, outputs as hex.
The script also runs the Python model on every case and stops on a difference, and decrypts every prg-ae case back."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import refgen  # noqa: E402
import orc_bashprg as M  # noqa: E402

L = refgen.ref()
_sz = ctypes.c_size_t
L.bashPrg_keep.restype = _sz


def ref_start(l, d, ann, key):
    st = ctypes.create_string_buffer(L.bashPrg_keep())
    L.bashPrgStart(st, _sz(l), _sz(d), bytes(ann), _sz(len(ann)), bytes(key), _sz(len(key)))
    return st


def ref_hash(l, d, ann, msg, out_len):
    st = ref_start(l, d, ann, b"")
    L.bashPrgAbsorb(bytes(msg), _sz(len(msg)), st)
    out = ctypes.create_string_buffer(out_len)
    L.bashPrgSqueeze(out, _sz(out_len), st)
    return out.raw


def ref_ae(decr, l, d, key, ann, hdr, text, tag_len):
    st = ref_start(l, d, ann, key)
    L.bashPrgAbsorb(bytes(hdr), _sz(len(hdr)), st)
    buf = ctypes.create_string_buffer(bytes(text), max(len(text), 1))
    (L.bashPrgDecr if decr else L.bashPrgEncr)(buf, _sz(len(text)), st)
    tag = ctypes.create_string_buffer(tag_len)
    L.bashPrgSqueeze(tag, _sz(tag_len), st)
    return buf.raw[:len(text)], tag.raw


def ref_case(c, x):
    if c["kind"] == "hash":
        return {"out": ref_hash(c["l"], c["d"], x["ann"], x["msg"], c["out_len"]).hex()}
    ct, tag = ref_ae(False, c["l"], c["d"], x["key"], x["ann"], x["hdr"], x["text"], c["tag_len"])
    pt, tag2 = ref_ae(True, c["l"], c["d"], x["key"], x["ann"], x["hdr"], ct, c["tag_len"])
    assert pt == x["text"] and tag2 == tag
    return {"ct": ct.hex(), "tag": tag.hex()}


def main():
    H = refgen.beltH()
    vectors = []
    for name, l, d, n, out_len in (("A.5.1", 128, 2, 0, 32), ("A.5.2", 128, 2, 127, 32), ("A.5.3", 128, 2, 128, 32),
                                   ("A.5.4", 128, 2, 150, 32), ("A.5.5", 192, 1, 143, 48), ("A.5.6", 192, 1, 144, 48),
                                   ("A.5.7", 192, 1, 150, 48)):
        c = {"name": name, "kind": "hash", "l": l, "d": d, "ann": "", "msg": H[:n].hex(), "out_len": out_len}
        vectors.append(c)
    vectors.append({"name": "A.6", "kind": "ae", "l": 256, "d": 1, "ann": H[:16].hex(), "key": H[32:64].hex(),
                    "hdr": H[64:64 + 49].hex(), "text": bytes(192).hex(), "tag_len": 32})
    for c in vectors:
        x = {k: bytes.fromhex(c[k]) for k in ("ann", "msg", "key", "hdr", "text") if k in c}
        got = ref_case(c, x)
        assert M.run_case(c, x) == got, c["name"]
        c.update(got)
    rnd = M.random_cases(0xBA5F, 204)
    for c in rnd:
        x = M.case_inputs(c)
        got = ref_case(c, x)
        assert M.run_case(c) == got, c
        c.update(got)
    path = os.path.join(ROOT, "tests", "golden", "bash_prg.json")
    with open(path, "w") as f:
        json.dump({"vectors": vectors, "random": rnd}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes;", len(vectors), "vectors,", len(rnd), "random cases")


if __name__ == "__main__":
    main()
