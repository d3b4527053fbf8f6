"""CPU tests of tests/golden/bign_steered.json (tools/make_golden_steered.py; tests/steered.py reads it): the fixture IS what its
families say -- u recomputed from every signature, the zero windows, the octets of s0, the step at which the model of the walk meets
T == +-E -- no family is empty, the oracle (and the reference, where it is built) gives every recorded code, and the HOST path of
the drop-in layer (bee2_amd/csrc/host_bign.hpp through tests/hostshim/host_bign_shim.cpp, as tests/test_host_bign.py builds it)
gives them too, with the oracle's x_R on the valid ones: its wNAF walk with u = 0, 1, q - 1 and the rest."""
import ctypes
import os
import re
import subprocess

import pytest

import refgen
import steered as ST
from conftest import hostshim_san_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    return ST.load()


@pytest.fixture(scope="module")
def hb(tmp_path_factory, orc):
    out = tmp_path_factory.mktemp("hostshim") / "libhostbign.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror"] + hostshim_san_flags() + ["-o", str(out),
                           os.path.join(ROOT, "tests", "hostshim", "host_bign_shim.cpp")])
    lib = ctypes.CDLL(str(out))
    lib.hb_verify.restype = ctypes.c_uint32
    lib.hb_init(orc.beltH())
    return lib


def _oid(l):
    from bee2_amd.engine import LEVEL_OID
    return bytes(LEVEL_OID[l])


def _zero_windows(c):
    return [j for j, w in enumerate(ST.windows16(c["U"], c["l"])) if w == 0]


@pytest.mark.parametrize("l", ST.LEVELS)
def test_every_case_has_the_declared_u(fx, l):
    q = fx.q[l]
    assert q >> (2 * l - 1) == 1
    for c in fx.of(l):
        assert len(c["hash"]) == l // 4 and len(c["sig"]) == 3 * l // 8 and len(c["pubkey"]) == l // 2
        assert ST.le(c["sig"][l // 8:]) < q, c["name"]                     # s1 in range: the verdict is the walk's
        assert ST.u_of(l, q, c["hash"], c["sig"]) == c["U"] < q, c["name"]
        assert ST.from_windows16(ST.windows16(c["U"], l)) == c["U"]
        ST.v_digits(ST.v_of(l, c["sig"]), l)


@pytest.mark.parametrize("l", ST.LEVELS)
def test_case_counts(fx, l):
    nw = ST.nw(l)
    count = {f: len(fx.of(l, f)) for f in ST.FAMILIES}
    assert count["a"] >= nw + 7 and count["b"] >= nw + 10 and count["c"] == 7 and count["d"] == 7
    assert count["e"] >= 2 * count["b"] + 1
    names = [c["name"] for c in fx.of(l)]
    assert len(set(names)) == len(names)
    by_parent = {}
    for c in fx.of(l, "e"):
        by_parent.setdefault(c["parent"], []).append(c)
    for b in fx.of(l, "b"):
        assert len(by_parent[b["name"]]) >= 2, b["name"]
        assert len({x["sig"] for x in by_parent[b["name"]]}) == len(by_parent[b["name"]])
    assert "u=0" in by_parent


@pytest.mark.parametrize("l", ST.LEVELS)
def test_family_a_extremes_of_u(fx, l):
    q, nw = fx.q[l], ST.nw(l)
    us = {c["U"] for c in fx.of(l, "a")}
    assert {0, 1, 2, q - 1, q - 2} <= us
    assert {1 << (16 * j) for j in range(nw)} <= us
    top = max(j for j in range(nw) if 0xFFFF << (16 * j) < q)
    assert {0xFFFF << (16 * j) for j in (0, nw // 2, top)} <= us
    assert all(c["code"] == 0 for c in fx.of(l, "a"))


@pytest.mark.parametrize("l", ST.LEVELS)
def test_family_b_zero_windows_of_u(fx, l):
    nw = ST.nw(l)
    zs = [frozenset(_zero_windows(c)) for c in fx.of(l, "b")]
    want = [frozenset({j}) for j in range(nw)] + [frozenset(range(nw // 2)), frozenset(range(nw // 2, nw))]
    want += [frozenset(j for j in range(nw) if j % 4 == r) for r in range(4)]
    want += [frozenset(j for j in range(nw) if j % 4 != r) for r in range(4)]
    assert set(want) <= set(zs)
    assert all(c["code"] == 0 for c in fx.of(l, "b"))


@pytest.mark.parametrize("l", ST.LEVELS)
def test_family_c_windows_of_v_under_one_key(fx, l):
    cs = fx.of(l, "c")
    half = l // 8
    assert {c["key_index"] for c in cs} == {0} and {c["pubkey"] for c in cs} == {fx.signers[l][0]["pubkey"]}
    assert fx.signers[l][0]["d"] is None and len(fx.signers[l][0]["pool"]) >= 10
    w8 = [ST.s0_windows8(l, c["sig"]) for c in cs]
    w16 = [ST.s0_windows16(l, c["sig"]) for c in cs]
    assert len(w8[0]) == half and len(w16[0]) == half // 2
    for i in (0, half // 2, half - 1):
        assert any(w[i] == 0 for w in w8), i                 # an empty 8-bit window at either end and in the middle
    for i in (0, half // 2 - 1):
        assert any(w[i] == 0 for w in w16), i                # an empty 16-bit window at either end
    assert any(w[-1] == 0xFF for w in w8) and sum(w[-1] == 0 for w in w8) >= 2
    for c in cs:                                             # ... each where its name says
        m = re.fullmatch(r"s0 (octet|word|top octet) (\w+)(?: zero)?", c["name"])
        kind, arg = m.group(1), m.group(2)
        if kind == "octet":
            assert ST.s0_windows8(l, c["sig"])[int(arg)] == 0
        elif kind == "word":
            assert ST.s0_windows16(l, c["sig"])[int(arg)] == 0
        else:
            assert ST.s0_windows8(l, c["sig"])[-1] == int(arg, 16)
    assert all(c["code"] == 0 for c in cs)


@pytest.mark.parametrize("l", ST.LEVELS)
def test_family_d_the_model_meets_the_comb_point_at_the_named_step(fx, orc, l):
    q, nw = fx.q[l], ST.nw(l)
    seen = set()
    for c in fx.of(l, "d"):
        d, v = c["d"], ST.v_of(l, c["sig"])
        assert fx.signers[l][c["key_index"]]["pubkey"] == c["pubkey"] and fx.signers[l][c["key_index"]]["d"] == d
        assert orc.pubkey_calc(l, d.to_bytes(l // 4, "little")) == (0, c["pubkey"])           # Q = d G: the model's premise
        assert not _zero_windows(c)
        ev = ST.walk(l, q, c["U"], v, d)
        if c["name"] == "fold E":
            assert ev == [] and ST.fold(q, c["U"], v, d) == "E"
            k = 2 * c["U"] % q
        else:
            kind, j = re.fullmatch(r"(-?E) at w(\d+)", c["name"]).groups()
            j = int(j)
            assert ev[0] == (j, kind), (c["name"], ev)                    # there, and nowhere earlier
            assert ev[1:] == ([(j + 1, "O")] if kind == "-E" and j + 1 < nw else [])
            assert ST.fold(q, c["U"], v, d) is None or (kind, j) == ("-E", nw - 1)
            seen.add((kind, j))
            k = (c["U"] + v * d) % q
        # a signer's one-time key is never 0: the one record with R = O is not a signature, and the reference says so
        assert c["code"] == (0 if k else ST.ERR_BAD_SIG), c["name"]
        assert (k == 0) == (c["name"] == f"-E at w{nw - 1}")
    assert seen == {(kind, j) for kind in ("E", "-E") for j in (0, nw // 2, nw - 1)}


@pytest.mark.parametrize("l", ST.LEVELS)
def test_family_e_neighbours(fx, l):
    q = fx.q[l]
    by_name = {c["name"]: c for c in fx.of(l)}
    for c in fx.of(l, "e"):
        p = by_name[c["parent"]]
        assert c["hash"] == p["hash"] and c["pubkey"] == p["pubkey"] and c["sig"][:l // 8] == p["sig"][:l // 8]
        delta = (c["U"] - p["U"]) % q
        j = c["window"]
        if p["U"] == 0:
            assert delta == 1 and j == 0
        else:
            zero = _zero_windows(p)
            assert j in (zero[0], zero[-1]) and delta in (1 << (16 * j), 0xFFFF << (16 * j))
            assert _zero_windows(c) == [z for z in zero if z != j]       # that window alone changed
        assert c["code"] == ST.ERR_BAD_SIG and p["code"] == 0


@pytest.mark.parametrize("l", ST.LEVELS)
def test_oracle_and_reference_verdicts(fx, orc, l):
    cs = fx.of(l)
    got = orc.verify_batch_l(l, _oid(l), b"".join(c["hash"] for c in cs), b"".join(c["sig"] for c in cs), b"".join(c["pubkey"] for c in cs))
    assert got == [c["code"] for c in cs]
    pool = [(h, s, sg["pubkey"]) for sg in fx.signers[l] for h, s in sg["pool"]]
    assert orc.verify_batch_l(l, _oid(l), b"".join(x[0] for x in pool), b"".join(x[1] for x in pool), b"".join(x[2] for x in pool)) == [0] * len(pool)
    if refgen.have_ref():
        assert [refgen.verify_l(l, c["hash"], c["sig"], c["pubkey"]) for c in cs] == [c["code"] for c in cs]


@pytest.mark.skipif(not refgen.have_ref(), reason="oracle/_ref not built")
def test_the_generator_writes_the_committed_file(tmp_path, capsys):
    import make_golden_steered
    out = tmp_path / "bign_steered.json"
    make_golden_steered.main(str(out))
    capsys.readouterr()
    assert out.read_bytes() == open(ST.PATH, "rb").read()


@pytest.mark.parametrize("l", ST.LEVELS)
def test_host_path_verdicts_and_x_of_R(fx, orc, hb, l):
    orc.lib.orc_bignVerify_ex.restype = ctypes.c_uint32
    oid = _oid(l)
    for c in fx.of(l):
        rx, orx = ctypes.create_string_buffer(l // 4), ctypes.create_string_buffer(l // 4)
        code = hb.hb_verify(ctypes.c_size_t(l), oid, ctypes.c_size_t(len(oid)), c["hash"], c["sig"], c["pubkey"], rx)
        assert code == c["code"], (c["family"], c["name"])
        if c["code"] == 0:
            assert orc.lib.orc_bignVerify_ex(ctypes.c_size_t(l), oid, ctypes.c_size_t(len(oid)), c["hash"], c["sig"], c["pubkey"], orx) == 0
            assert rx.raw == orx.raw and any(orx.raw), (c["family"], c["name"])
