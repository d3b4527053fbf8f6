"""-m gpu: the bpki password containers as batches (bee2hip_bpkiUnwrap_batch / bee2hip_bpkiWrap_batch: belt-pbkdf2 into the
per-record-key belt-kwp inside the DER frames) against the reference's recorded outputs (tests/golden/bpki.json) and the
plain-Python model (tests/orc_bpki.py, which tests/test_bpki.py pins to that fixture).  One PBKDF2 launch costs its iteration
count whatever the batch holds, so each test makes few calls: about 0.25 s at 10000 iterations, 1.6 s at 65536."""
import json
import os
import random

import pytest

import bpkigrid as G
import orc_bpki as M
from bee2_amd import engine as E
from gpulib import engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "bpki.json")))


def check_unwrap(eng, kind, rows):
    """rows: [(container, password, expected code, expected key)] as one batch"""
    code, keys, codes, raw = eng.bpkiUnwrap_batch(kind, [r[0] for r in rows], [r[1] for r in rows])
    assert code == E.ERR_OK
    assert codes == [r[2] for r in rows], [(i, codes[i], rows[i][2]) for i in range(len(rows)) if codes[i] != rows[i][2]][:8]
    for i, r in enumerate(rows):
        assert keys[i] == r[3] and raw[64 * i:64 * i + 64] == r[3].ljust(64, b"\0"), i


@pytest.mark.parametrize("kind", [0, 1], ids=["privkey", "share"])
def test_the_whole_fixture_as_one_batch(fixture, kind):
    """every good container of the kind (all key lengths, both iteration counts, all password lengths), each once more under a
    password that differs in one bit, and the whole malformed corpus, interleaved: keys, lengths and codes are the reference's,
    refused slots are zero"""
    rows = []
    for r in fixture["good"]:
        if r["kind"] == kind:
            x, epki = G.case_inputs(r), bytes.fromhex(r["epki"])
            rows += [(epki, x["pwd"], E.ERR_OK, x["key"]), (epki, x["wrong_pwd"], r["wrong_code"], b"")]
    c = G.base_case(kind, fixture["good"])
    x, base = G.case_inputs(c), bytes.fromhex(c["epki"])
    bad = [(base[:r["len"]] if r["name"] == "trunc" else bytes.fromhex(r["epki"]), x["pwd"], r["code"], x["key"] if r["code"] == 0 else b"")
           for r in fixture["bad"] if r["kind"] == kind]
    assert len(rows) == 2 * (5 * len(M.KEY_LENS[kind]) + 2) and len(bad) > 190 and {r[2] for r in bad} >= {0, E.ERR_BAD_FORMAT, E.ERR_BAD_INPUT, E.ERR_BAD_KEYTOKEN}
    random.Random(kind).shuffle(bad)
    mixed = []
    while rows or bad:                                                # a good row, a few malformed ones, ...
        mixed += rows[:1] + bad[:5]
        rows, bad = rows[1:], bad[5:]
    check_unwrap(engine(), kind, mixed)


@pytest.mark.parametrize("kind", [0, 1], ids=["privkey", "share"])
def test_hand_built_frames_in_several_groups_against_the_model(kind):
    """130 containers at 1, 2, 3 and 1000 iterations -- bee2 opens what it would not seal -- of every key length, a fifth of them
    under a wrong password, one with a faulty inner frame: four PBKDF2 groups, one of 5 records, and several kwp runs"""
    rnd = random.Random(40 + kind)
    iters = [1] * 70 + [2] * 40 + [3] * 5 + [1000] * 15
    rnd.shuffle(iters)
    rows = []
    for i, it in enumerate(iters):
        key = bytearray(rnd.randbytes(M.KEY_LENS[kind][i % len(M.KEY_LENS[kind])]))
        key[0] = 1 + i % 16
        pwd, salt = rnd.randbytes(i % 41), rnd.randbytes(8)
        pki = G.pki_frame(kind, bytes(key), tail=b"\0") if i == 77 else None
        epki = M.epki_build(salt, it, M.seal(kind, bytes(key), pwd, salt, it, pki=pki))
        used = pwd + b"!" if i % 5 == 1 else pwd
        code, want = M.unwrap(kind, epki, used)
        assert code == (E.ERR_BAD_KEYTOKEN if i % 5 == 1 else E.ERR_BAD_FORMAT if i == 77 else 0)
        rows.append((epki, used, code, want))
    check_unwrap(engine(), kind, rows)


def test_nine_iteration_counts_are_refused_with_nothing_written():
    eng = engine()
    epkis = [M.epki_build(bytes(8), it, M.seal(0, bytes(32), b"p", bytes(8), it)) for it in range(1, 10)]
    code, keys, codes, raw = eng.bpkiUnwrap_batch(0, epkis, [b"p"] * 9)
    assert code == E.ERR_NOT_IMPLEMENTED and not any(raw) and codes == [0] * 9 and keys == [b""] * 9      # (the wrapper's zeroed buffers)
    code, keys, codes, raw = eng.bpkiUnwrap_batch(0, epkis[:8], [b"p"] * 8)
    assert code == E.ERR_OK and codes == [0] * 8 and keys == [bytes(32)] * 8


@pytest.mark.parametrize("kind", [0, 1], ids=["privkey", "share"])
def test_wrap_of_the_fixture_parts_equals_the_fixture_containers(fixture, kind):
    """one call per (key length, iteration count) of the fixture: every container octet for octet what the reference wrote"""
    eng = engine()
    groups = {}
    for r in fixture["good"]:
        if r["kind"] == kind:
            groups.setdefault((r["key_len"], r["iter"]), []).append(r)
    assert len(groups) == len(M.KEY_LENS[kind]) + 1
    for (key_len, iters), rows in groups.items():
        xs = [G.case_inputs(r) for r in rows]
        code, epkis = eng.bpkiWrap_batch(kind, [x["key"] for x in xs], [x["pwd"] for x in xs], [x["salt"] for x in xs], iters)
        assert code == E.ERR_OK and [e.hex() for e in epkis] == [r["epki"] for r in rows], (key_len, iters)


@pytest.mark.parametrize("kind", [0, 1], ids=["privkey", "share"])
def test_wrap_then_unwrap_of_130_records(kind):
    eng = engine()
    rnd = random.Random(60 + kind)
    key_len = M.KEY_LENS[kind][-1]
    keys = [bytes([1 + i % 16]) + rnd.randbytes(key_len - 1) for i in range(130)]
    pwds, salts = [rnd.randbytes(i % 67) for i in range(130)], [rnd.randbytes(8) for _ in range(130)]
    code, epkis = eng.bpkiWrap_batch(kind, keys, pwds, salts, 10000)
    assert code == E.ERR_OK and len(epkis) == 130 and len({len(e) for e in epkis}) == 1
    for i in (0, 64, 129):                                            # three of them against the model, the rest by their frames
        assert M.wrap(kind, keys[i], pwds[i], salts[i], 10000) == (E.ERR_OK, epkis[i]), i
    for i in range(130):
        assert M.epki_parse(epkis[i])[:2] == (salts[i], 10000)
    pwds[7] += b"x"
    code, got, codes, _ = eng.bpkiUnwrap_batch(kind, epkis, pwds)
    assert code == E.ERR_OK and codes == [E.ERR_BAD_KEYTOKEN if i == 7 else 0 for i in range(130)]
    assert got == [b"" if i == 7 else keys[i] for i in range(130)]
