"""tests/golden/bpki.json: password-protected containers with the reference's own outputs (oracle/_ref/libbee2ref.so:
bpkiPrivkeyWrap / bpkiPrivkeyUnwrap / bpkiShareWrap / bpkiShareUnwrap, src/crypto/bpki.c).  Build container only.

  * "good": tests/bpkigrid.py good_cases(); inputs come from each row's seed.  Per row: the container the reference writes, and
    the code of opening it with a password that differs in one bit.  The script opens every container with the reference again.
  * "bad": the malformed corpus of each kind, derived from bpkigrid.base_case(kind) and opened with that row's password, with the
    reference's code for every row: {"kind", "name", "epki"} or, for a truncation, {"kind", "name": "trunc", "len"}.  The rows
    named inner_* hold a faulty inner frame sealed again with tests/orc_beltkwp.py under the password's key, so that belt-kwp
    accepts them.
A row whose iteration count the reference would really run (an INTEGER of nine octets with a zero in front) is not here: the
batch refuses it by its own limit, which tests/test_bpki.py checks without the reference."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import refgen  # noqa: E402
import bpkigrid as G  # noqa: E402
import orc_bpki as M  # noqa: E402

L = refgen.ref()
_sz = ctypes.c_size_t
WRAP, UNWRAP = (L.bpkiPrivkeyWrap, L.bpkiShareWrap), (L.bpkiPrivkeyUnwrap, L.bpkiShareUnwrap)


def ref_wrap(kind, key, pwd, salt, iters):
    n = _sz(0)
    assert WRAP[kind](None, ctypes.byref(n), key, _sz(len(key)), pwd, _sz(len(pwd)), salt, _sz(iters)) == 0
    out = ctypes.create_string_buffer(n.value)
    assert WRAP[kind](out, ctypes.byref(n), key, _sz(len(key)), pwd, _sz(len(pwd)), salt, _sz(iters)) == 0
    return out.raw


def ref_unwrap(kind, epki, pwd):
    out, n = ctypes.create_string_buffer(64), _sz(0)
    buf = ctypes.create_string_buffer(bytes(epki), max(len(epki), 1))          # (an exact copy: nothing of ours behind it)
    code = UNWRAP[kind](out, ctypes.byref(n), buf, _sz(len(epki)), pwd, _sz(len(pwd)))
    return code, out.raw[:n.value] if code == 0 else b""


def main():
    good = G.good_cases()
    for c in good:
        x = G.case_inputs(c)
        epki = ref_wrap(c["kind"], x["key"], x["pwd"], x["salt"], c["iter"])
        assert ref_unwrap(c["kind"], epki, x["pwd"]) == (0, x["key"]), c
        c.update(epki=epki.hex(), wrong_code=ref_unwrap(c["kind"], epki, x["wrong_pwd"])[0])
    bad = []
    for kind in (0, 1):
        c = G.base_case(kind, good)
        x = G.case_inputs(c)
        epki = bytes.fromhex(c["epki"])
        salt, iters, off, n = M.epki_parse(epki)
        for k in range(len(epki)):
            bad.append({"kind": kind, "name": "trunc", "len": k, "code": ref_unwrap(kind, epki[:k], x["pwd"])[0]})
        rows = G.outer_variants(salt, iters, epki[off:off + n])
        rows += [(name, M.epki_build(salt, iters, M.seal(kind, None, x["pwd"], salt, iters, pki=pki)))
                 for name, pki in G.inner_variants(kind, x["key"])]
        for name, e in rows:
            bad.append({"kind": kind, "name": name, "epki": e.hex(), "code": ref_unwrap(kind, e, x["pwd"])[0]})
    path = os.path.join(ROOT, "tests", "golden", "bpki.json")
    with open(path, "w") as f:
        json.dump({"good": good, "bad": bad}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes;", len(good), "good rows,", len(bad), "malformed rows")


if __name__ == "__main__":
    main()
