"""CPU tests of the belt-dwp / belt-che record batch (include/bee2hip.h, bee2_amd/csrc/capi_beltae.hip): every refusal
answers before any device work, the C oracle that the GPU tests compare against reproduces the reference's records of
tests/golden/belt_ae_ragged.json, the carry record carries, and the grid batches cover what they claim."""
import ctypes
import json
import os

import pytest

import beltaegrid as G
import bee2_amd
import refgen
from bee2_amd import engine as E
from raggedgrid import missing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_sz, _vp, _int = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int
NAMES = ["bee2hip_beltAE_wrap_ragged", "bee2hip_beltAE_unwrap_ragged", "bee2hip_beltAE_ragged_stream"]


@pytest.fixture(scope="module")
def fixtures():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "belt_ae_ragged.json")))


# ---- argument checks: none of these calls may reach a device (no GPU here), and none dereferences a device pointer -- the
# device "pointers" are made-up addresses with the alignment the header grants
A8, A4 = 0x7000_0000_1000, 0x7000_0000_2004


def _stream(lib, unwrap=0, mode=0, key_len=32, ivs=A4 + 1, hdrs=A4 + 3, hoff=A8, src=A4 + 1, off=A8, order=A4, n=4, dst=A4 + 2,
            tags=A4 + 3, codes=A4, key=bytes(32)):
    return lib.bee2hip_beltAE_ragged_stream(_int(unwrap), _int(mode), key, _sz(key_len), _vp(ivs), _vp(hdrs), _vp(hoff), _vp(src),
                                            _vp(off), _vp(order), _sz(n), _vp(dst), _vp(tags), _vp(codes), None)


def _q(*xs):
    return (ctypes.c_uint64 * len(xs))(*xs)


def _host(lib, unwrap, mode=0, key_len=32, n=1 << 32, key=bytes(32), ivs=bytes(64), hdrs=None, hoff=None, src=bytes(64),
          off=_q(0, 0, 0, 0, 0), dst=None, tags=None, codes=None):
    dst = ctypes.create_string_buffer(64) if dst is None else dst
    tags = ctypes.create_string_buffer(64) if tags is None else tags
    codes = (ctypes.c_uint32 * 8)() if codes is None else codes
    if unwrap:
        return lib.bee2hip_beltAE_unwrap_ragged(_int(mode), key, _sz(key_len), ivs, hdrs, hoff, src, off, _sz(n), tags, dst, codes)
    return lib.bee2hip_beltAE_wrap_ragged(_int(mode), key, _sz(key_len), ivs, hdrs, hoff, src, off, _sz(n), dst, tags)


def test_every_refusal_answers_without_a_device():
    lib = bee2_amd.load().lib
    for name in NAMES:
        getattr(lib, name).restype = ctypes.c_uint32
    entries = [lambda **k: _stream(lib, 0, **k), lambda **k: _stream(lib, 1, **k), lambda **k: _host(lib, 0, **k),
               lambda **k: _host(lib, 1, **k)]
    for f in entries:
        # every other argument valid; for the host entries n = 2^32 is itself refused, so each line names one cause only
        # through the order of the checks: key and mode first
        for key_len in (0, 1, 8, 15, 17, 20, 31, 33, 48, 64):
            assert f(key_len=key_len, n=4) == E.ERR_BAD_INPUT, key_len
        for mode in (-1, 2, 3, 256):
            assert f(mode=mode, n=4) == E.ERR_BAD_INPUT, mode
        assert f(key=None, n=4) == E.ERR_BAD_INPUT
        assert f(n=1 << 32) == E.ERR_BAD_INPUT
        assert f(n=(1 << 32) + 5) == E.ERR_BAD_INPUT
        for key_len in G.KEY_LENS:
            for mode in G.MODES:
                assert f(key_len=key_len, mode=mode, n=0) == E.ERR_OK           # an empty batch is nothing to do
    for unwrap in (-1, 2):
        assert _stream(lib, unwrap) == E.ERR_BAD_INPUT
    # alignment of the device pointers: offsets 8, order / codes 4; ivs, headers, text and tags 1
    for u in (0, 1):
        for bad in (1, 2, 4):
            assert _stream(lib, u, off=A8 + bad) == E.ERR_BAD_INPUT
            assert _stream(lib, u, hoff=A8 + bad) == E.ERR_BAD_INPUT
        for bad in (1, 2, 3):
            assert _stream(lib, u, order=A4 + bad) == E.ERR_BAD_INPUT
            assert _stream(lib, u, codes=A4 + bad) == E.ERR_BAD_INPUT
    # missing buffers, as bee2hip_bashPrgAE_ragged_stream refuses them
    assert _stream(lib, 0, off=None) == E.ERR_BAD_INPUT and _stream(lib, 0, tags=None) == E.ERR_BAD_INPUT
    assert _stream(lib, 0, ivs=None) == E.ERR_BAD_INPUT and _stream(lib, 1, codes=None) == E.ERR_BAD_INPUT
    assert _stream(lib, 0, hoff=None) == E.ERR_BAD_INPUT                        # headers without their offsets
    assert _stream(lib, 0, dst=None) == E.ERR_BAD_INPUT and _stream(lib, 1, src=None) == E.ERR_BAD_INPUT
    # ... and as prg_ae_host does; decreasing offsets
    for u in (0, 1):
        ok = dict(n=3, off=_q(0, 5, 5, 9))
        assert _host(lib, u, n=3, off=None) == E.ERR_BAD_INPUT
        assert _host(lib, u, n=3, off=_q(0, 5, 4, 9)) == E.ERR_BAD_INPUT
        assert _host(lib, u, n=3, off=_q(7, 5, 9, 9)) == E.ERR_BAD_INPUT
        assert _host(lib, u, hdrs=bytes(16), hoff=_q(0, 3, 2, 4), **ok) == E.ERR_BAD_INPUT
        assert _host(lib, u, hdrs=bytes(16), hoff=None, **ok) == E.ERR_BAD_INPUT
        assert _host(lib, u, hdrs=None, hoff=_q(0, 3, 3, 4), **ok) == E.ERR_BAD_INPUT       # header octets and nowhere to read them
        assert _host(lib, u, ivs=None, **ok) == E.ERR_BAD_INPUT
        assert _host(lib, u, src=None, **ok) == E.ERR_BAD_INPUT
    for what in ("tags", "dst"):
        for u in (0, 1):
            assert _host(lib, u, n=3, off=_q(0, 5, 5, 9), **{what: ctypes.c_char_p(None)}) == E.ERR_BAD_INPUT, what
    assert _host(lib, 1, n=3, off=_q(0, 5, 5, 9), codes=ctypes.POINTER(ctypes.c_uint32)()) == E.ERR_BAD_INPUT


def test_interface_lists_the_three_entries():
    assert set(NAMES) <= set(E.BATCH_SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "bee2hip.h")).read()
    assert all(n + "(" in hdr for n in NAMES)
    assert set(NAMES) <= E.lib_exports()
    # the difference from beltDWPUnwrap / beltCHEUnwrap is stated where callers read: in the comment above the entries, and it
    # names bee2, the refused record and the zeros (whatever the wording)
    import re
    at = hdr.index("err_t bee2hip_beltAE_wrap_ragged(")
    comment = hdr[hdr.rindex("/*", 0, at):at].lower()
    assert "bee2" in comment and "unwrap" in comment and "refuse" in comment and re.search(r"\bzeros?\b", comment)
    assert "differen" in comment


# ---- the fixture: the reference's own outputs, and the oracle reproduces them
def test_fixture_spans_modes_key_lengths_and_the_grid_lengths(fixtures):
    recs = fixtures["records"]
    assert [{k: c[k] for k in ("mode", "key_len", "text_len", "hdr_len", "seed")} for c in recs] == G.fixture_cases()
    assert len(recs) >= 300
    assert {(c["mode"], c["key_len"]) for c in recs} == {(m, k) for m in G.MODES for k in G.KEY_LENS}
    for m in G.MODES:
        for k in G.KEY_LENS:
            assert {c["text_len"] for c in recs if (c["mode"], c["key_len"]) == (m, k)} == set(G.TEXT_LENS)
    assert {c["hdr_len"] for c in recs} == set(G.HDR_LENS)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "belt_ae_ragged.json")) < 300_000


def test_oracle_reproduces_every_fixture_record(fixtures, orc):
    for c in fixtures["records"]:
        x = G.case_inputs(c)
        mode = G.MODES[c["mode"]]
        code, ct, tag = orc.dwp_wrap(x["text"], x["hdr"], x["key"], x["iv"], mode)
        assert code == 0 and ct.hex() == c["ct"] and tag.hex() == c["tag"], c
        code, pt = orc.dwp_unwrap(ct, x["hdr"], tag, x["key"], x["iv"], mode)
        assert code == 0 and pt == x["text"], c
        bad = bytes([tag[0] ^ 1]) + tag[1:]
        assert orc.dwp_unwrap(ct, x["hdr"], bad, x["key"], x["iv"], mode)[0] == G.ERR_BAD_MAC


def test_carry_record_carries_out_of_the_low_word_and_the_oracle_follows(fixtures, orc):
    c = fixtures["carry"]
    x = G.carry_inputs(c["iv"])
    low = G.carry_counter(orc, x["iv"])
    assert low >= (1 << 32) - (1 << 12)                          # s + j passes 2^32 for some j <= 2^12 ...
    assert len(x["text"]) == 16 * G.CARRY_BLOCKS and G.CARRY_BLOCKS > (1 << 32) - low          # ... inside the record
    code, ct, tag = orc.dwp_wrap(x["text"], x["hdr"], x["key"], x["iv"], "DWP")
    assert code == 0 and tag.hex() == c["tag"] and G.sha(ct) == c["ct_sha256"]


@pytest.mark.ref
@pytest.mark.skipif(not refgen.have_ref(), reason="oracle/_ref not built")
def test_fixture_is_what_the_reference_gives_now(fixtures):
    import make_golden_beltae as mg
    for c in fixtures["records"][::7]:
        x = G.case_inputs(c)
        ct, tag = mg.ref_wrap(c["mode"], x["key"], x["iv"], x["hdr"], x["text"])
        assert (ct.hex(), tag.hex()) == (c["ct"], c["tag"])


# ---- the grid
@pytest.mark.parametrize("mode", sorted(G.MODES))
def test_grid_holds_every_length_at_every_start_alignment(mode):
    b = G.grid(mode)
    assert set(range(0, 50)) | {63, 64, 65, 127, 128, 129, 255, 256, 257} == set(G.TEXT_LENS)
    assert {L % 16 for L in G.TEXT_LENS} == set(range(16))
    assert not missing(b.offsets, G.TEXT_LENS)
    assert b.n == 2 * 16 * len(G.TEXT_LENS)
    assert G.header_coverage(b) >= {(s, h) for s in G.HDR_RES for h in G.HDR_LENS}
    assert len(b.ivs) == 16 * b.n and len(set(b.iv(i) for i in range(b.n))) == b.n


def test_edge_batches_straddle_the_bucketing_threshold():
    for n in (1, 63, 64, 65, 127, 128, 129, 1025):
        b = G.edge(n, n % 2, G.KEY_LENS[n % 3])
        lens = [b.offsets[i + 1] - b.offsets[i] for i in range(n)]
        assert b.n == n and (n < 63 or set(G.LONG) <= set(lens))
        assert n < 63 or 0 in lens
