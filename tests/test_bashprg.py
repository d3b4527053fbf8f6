"""CPU tests of the bash-prg batch entries (include/bee2hip.h, bee2_amd/csrc/capi_prg.hip): the Python model that the GPU
tests compare against is pinned to the reference's fixtures, the grid batches cover what they claim, and every parameter
and alignment error answers before any device work."""
import ctypes
import json
import os
import random

import pytest

import bashprggrid as G
import bee2_amd
import orc_bashprg as M
import refgen
from bee2_amd import engine as E
from raggedgrid import missing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_sz, _vp = ctypes.c_size_t, ctypes.c_void_p


@pytest.fixture(scope="module")
def fixtures():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "bash_prg.json")))


def test_model_gives_the_standards_vectors(fixtures):
    """STB 34.101.77 A.5.1 - A.5.7 and A.6 as the reference computes them (test/crypto/bash_test.c)"""
    names = [v["name"] for v in fixtures["vectors"]]
    assert names == [f"A.5.{k}" for k in range(1, 8)] + ["A.6"]
    for v in fixtures["vectors"]:
        x = {k: bytes.fromhex(v[k]) for k in ("ann", "msg", "key", "hdr", "text") if k in v}
        got = M.run_case(v, x)
        assert all(got[k] == v[k] for k in got), v["name"]
    a6 = fixtures["vectors"][-1]
    code, pt = M.ae_unwrap(256, 1, bytes.fromhex(a6["key"]), bytes.fromhex(a6["ann"]), bytes.fromhex(a6["hdr"]),
                           bytes.fromhex(a6["ct"]), bytes.fromhex(a6["tag"]))
    assert code == M.ERR_OK and pt == bytes(192)


def test_model_equals_every_random_fixture_case(fixtures):
    cases = fixtures["random"]
    assert len(cases) >= 200 and {(c["l"], c["d"]) for c in cases} == set(M.LD)
    assert {c["ann_len"] for c in cases} == {0, 4, 16, 60}
    for c in cases:
        got = M.run_case(c)
        assert all(got[k] == c[k] for k in got), c
        if c["kind"] == "ae":
            x = M.case_inputs(c)
            code, pt = M.ae_unwrap(c["l"], c["d"], x["key"], x["ann"], x["hdr"], bytes.fromhex(c["ct"]), bytes.fromhex(c["tag"]))
            assert code == M.ERR_OK and pt == x["text"]


@pytest.mark.ref
@pytest.mark.skipif(not refgen.have_ref(), reason="oracle/_ref not built")
def test_model_equals_the_reference_live_on_a_fresh_seed():
    import make_golden_bashprg as mg
    for c in M.random_cases(random.SystemRandom().randrange(1 << 32), 60):
        x = M.case_inputs(c)
        assert M.run_case(c) == mg.ref_case(c, x), c


@pytest.mark.parametrize("l,d", M.LD)
def test_grid_batches_hold_every_length_at_every_start_alignment(l, d):
    """as tests/test_ragged_grid.py: every (offset mod 16, length) pair of the grid is a record of the batch, the headers
    cycle through 0, 1, r-1, r, r+1 and the four configurations span the announcement, key and tag lengths"""
    for keyed, grid in ((True, G.ae_grid), (False, G.hash_grid)):
        r = M.rate(l, d, keyed)
        lengths = G.grid_lengths(r)
        assert set(range(0, r + 18)) | {2 * r - 1, 2 * r, 2 * r + 1} | set(range(3 * r - 16, 3 * r + 2)) == set(lengths)
        for c in range(4):
            b = grid(l, d, c)
            assert not missing(b.offsets, lengths)
            assert b.n == 2 * 16 * len(lengths)
            if keyed:
                hl = {b.hoffsets[i + 1] - b.hoffsets[i] for i in range(b.n)}
                assert hl == {0, 1, r - 1, r, r + 1}
                assert {(b.hoffsets[i] % 16) for i in range(b.n)} == set(range(16))
    assert {G.grid_config(l, c)[0] for c in range(4)} == {0, 4, 16, 60}
    assert {G.grid_config(l, c)[2] for c in range(4)} == {1, 8, 32, 64}
    ks = [G.grid_config(l, c)[1] for c in range(4)]
    assert ks[0] == l // 8 and ks[-1] == 60 and all(k % 4 == 0 for k in ks)


def test_rates_are_those_of_the_reference_table():
    """bash_prg.c:34-43"""
    want = {(128, 1): (168, 160), (128, 2): (160, 128), (192, 1): (156, 144), (192, 2): (144, 96), (256, 1): (144, 128),
            (256, 2): (128, 64)}
    assert {ld: (M.rate(*ld, True), M.rate(*ld, False)) for ld in M.LD} == want


# ---- argument checks: none of these calls may reach a device (no GPU here), and none dereferences a pointer -- the device
# "pointers" are made-up addresses with the alignment the header grants
A8, A4 = 0x7000_0000_1000, 0x7000_0000_2004


def _hash_stream(lib, l=128, d=2, ann_len=0, off=A8, order=A4, n=4, out=A4, out_len=32, data=A4 + 1):
    return lib.bee2hip_bashPrgHash_ragged_stream(_sz(l), _sz(d), bytes(64), _sz(ann_len), _vp(data), _vp(off), _vp(order), _sz(n),
                                                 _vp(out), _sz(out_len), None)


def _ae_stream(lib, unwrap=0, l=128, d=2, key_len=32, anns=A4, ann_len=16, hdrs=A4 + 3, hoff=A8, src=A4 + 1, off=A8, order=A4, n=4,
               dst=A4 + 2, tags=A4 + 3, tag_len=8, codes=A4):
    return lib.bee2hip_bashPrgAE_ragged_stream(ctypes.c_int(unwrap), _sz(l), _sz(d), bytes(64), _sz(key_len), _vp(anns),
                                               _sz(ann_len), _vp(hdrs), _vp(hoff), _vp(src), _vp(off), _vp(order), _sz(n), _vp(dst),
                                               _vp(tags), _sz(tag_len), _vp(codes), None)


def _hash_host(lib, l=128, d=2, ann_len=0, n=1 << 32, out_len=32):
    return lib.bee2hip_bashPrgHash_ragged(_sz(l), _sz(d), bytes(64), _sz(ann_len), bytes(16), bytes(16), _sz(n), bytes(64),
                                          _sz(out_len))


def _ae_host(lib, unwrap, l=128, d=2, key_len=32, ann_len=16, n=1 << 32, tag_len=8):
    if unwrap:
        return lib.bee2hip_bashPrgAE_unwrap_ragged(_sz(l), _sz(d), bytes(64), _sz(key_len), bytes(64), _sz(ann_len), None, None,
                                                   bytes(16), bytes(16), _sz(n), bytes(64), _sz(tag_len), bytes(16), bytes(16))
    return lib.bee2hip_bashPrgAE_wrap_ragged(_sz(l), _sz(d), bytes(64), _sz(key_len), bytes(64), _sz(ann_len), None, None, bytes(16),
                                             bytes(16), _sz(n), bytes(16), bytes(64), _sz(tag_len))


def test_parameter_and_alignment_errors_need_no_device():
    lib = bee2_amd.load().lib
    entries = [_hash_stream, lambda lib, **k: _ae_stream(lib, 0, **k), lambda lib, **k: _ae_stream(lib, 1, **k), _hash_host,
               lambda lib, **k: _ae_host(lib, 0, **k), lambda lib, **k: _ae_host(lib, 1, **k)]
    keyed = entries[1:3] + entries[4:]
    # l and d: ERR_BAD_PARAMS from every entry (every other argument valid; for the host entries n = 2^32 would be the
    # next complaint, so a wrong order of the checks shows as ERR_BAD_INPUT)
    for f in entries:
        for l in (0, 64, 127, 160, 224, 320, 512):
            assert f(lib, l=l) == E.ERR_BAD_PARAMS, l
        for d in (0, 3, 4):
            assert f(lib, d=d) == E.ERR_BAD_PARAMS, d
        for ann_len in (1, 2, 3, 6, 61, 62, 63, 64, 128):
            assert f(lib, ann_len=ann_len) == E.ERR_BAD_INPUT, ann_len
        assert f(lib, n=1 << 32) == E.ERR_BAD_INPUT
    for f in (_hash_stream, _hash_host):
        for out_len in (0, 65, 128):
            assert f(lib, out_len=out_len) == E.ERR_BAD_INPUT, out_len
    for f in keyed:
        for tag_len in (0, 65, 128):
            assert f(lib, tag_len=tag_len) == E.ERR_BAD_INPUT, tag_len
        for l in (128, 192, 256):
            for key_len in (0, 4, l // 8 - 4, l // 8 + 1, l // 8 + 2, 61, 62, 63, 64):
                assert f(lib, l=l, key_len=key_len) == E.ERR_BAD_INPUT, (l, key_len)
    # alignment of the device pointers: offsets 8, order / anns / codes 4
    for bad in (1, 2, 4):
        assert _hash_stream(lib, off=A8 + bad) == E.ERR_BAD_INPUT
        for u in (0, 1):
            assert _ae_stream(lib, u, off=A8 + bad) == E.ERR_BAD_INPUT
            assert _ae_stream(lib, u, hoff=A8 + bad) == E.ERR_BAD_INPUT
    for bad in (1, 2, 3):
        assert _hash_stream(lib, order=A4 + bad) == E.ERR_BAD_INPUT
        for u in (0, 1):
            assert _ae_stream(lib, u, order=A4 + bad) == E.ERR_BAD_INPUT
            assert _ae_stream(lib, u, anns=A4 + bad) == E.ERR_BAD_INPUT
            assert _ae_stream(lib, u, codes=A4 + bad) == E.ERR_BAD_INPUT
    # missing buffers
    assert _hash_stream(lib, off=None) == E.ERR_BAD_INPUT and _hash_stream(lib, out=None) == E.ERR_BAD_INPUT
    assert _ae_stream(lib, 0, tags=None) == E.ERR_BAD_INPUT and _ae_stream(lib, 0, anns=None) == E.ERR_BAD_INPUT
    assert _ae_stream(lib, 1, codes=None) == E.ERR_BAD_INPUT and _ae_stream(lib, 0, hoff=None) == E.ERR_BAD_INPUT
    assert _ae_stream(lib, 0, dst=None) == E.ERR_BAD_INPUT and _ae_stream(lib, 2) == E.ERR_BAD_INPUT
    # an empty batch is nothing to do, with or without a device
    assert _hash_host(lib, n=0) == E.ERR_OK and _ae_host(lib, 0, n=0) == E.ERR_OK and _ae_host(lib, 1, n=0) == E.ERR_OK


def test_python_interface_lists_the_five_entries():
    names = ["bee2hip_bashPrgHash_ragged", "bee2hip_bashPrgAE_wrap_ragged", "bee2hip_bashPrgAE_unwrap_ragged",
             "bee2hip_bashPrgHash_ragged_stream", "bee2hip_bashPrgAE_ragged_stream"]
    assert set(names) <= set(E.BATCH_SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "bee2hip.h")).read()
    assert all(n + "(" in hdr for n in names)
    exported = E.lib_exports()
    assert set(names) <= exported
    assert not [s for s in exported if s.startswith("bashPrg")]          # bee2's own step functions are not taken over
