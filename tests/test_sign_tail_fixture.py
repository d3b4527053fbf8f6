"""CPU tests of tests/golden/bign_sign_tail.json (tools/make_golden_sign_tail.py; tests/signtail.py reads it and restates the tail of
signing in integers): every record IS what its kind and name say -- r, u, s1, the event of the fold and the borrows recomputed from
its octets --, the events the fixture witnesses are EXACTLY the ones the bound on the first fold leaves possible, and the oracle
gives every record's signature, public key and verdict.  The host path's signatures are held to the same records in
tests/test_host_bign_ct.py, the kernels' in tests/test_gpu_bign_sign_tail.py."""
import json
import re

import pytest

import refgen
import signtail as T

ERR_BAD_SIG = T.ERR_BAD_SIG


@pytest.fixture(scope="module")
def fx():
    return T.load()


def _claims(l, q):
    """name -> predicate over (t = the tail in integers, k, H): what the generator promised"""
    W = 1 << (2 * l)
    cq = W - q
    return {
        "fold": {"r=1": lambda t, k, H: t["r"] == 1 and t["event"][2] == 1, "r=2": lambda t, k, H: t["r"] == 2 and t["event"][2] == 1,
                 "r=cq-1": lambda t, k, H: t["r"] == cq - 1 and t["event"][2] == 1, "r=cq": lambda t, k, H: t["r"] == cq and t["event"][2] == 0,
                 "r=cq+1": lambda t, k, H: t["r"] == cq + 1 and t["event"][2] == 0, "r=q-2": lambda t, k, H: t["r"] == q - 2 and t["event"][2] == 0,
                 "r=q-1": lambda t, k, H: t["r"] == q - 1 and t["event"][2] == 0,
                 # taken, and k < r: a subtraction left out would show here and only here (k - (r + q) + q == k - r when k >= r)
                 "r=2 k=1": lambda t, k, H: (t["r"], k, t["u"], t["event"][2], t["borrow1"]) == (2, 1, q - 1, 1, 1),
                 "r=cq-1 k=cq-2": lambda t, k, H: (t["r"], k, t["u"], t["event"][2], t["borrow1"]) == (cq - 1, cq - 2, q - 1, 1, 1)},
        "sub1": {"u=0": lambda t, k, H: t["u"] == 0 and t["r"] == k and t["borrow1"] == 0,
                 "u=q-1": lambda t, k, H: t["u"] == q - 1 and t["r"] == k + 1 and t["borrow1"] == 1,
                 "u=1": lambda t, k, H: t["u"] == 1 and t["borrow1"] == 0,
                 "k=1 r=q-1": lambda t, k, H: k == 1 and t["r"] == q - 1 and t["u"] == 2 and t["borrow1"] == 1,
                 "k=q-1 r=1": lambda t, k, H: k == q - 1 and t["r"] == 1 and t["u"] == q - 2 and t["borrow1"] == 0},
        "sub2": {"s1=0": lambda t, k, H: H < q and t["s1"] == 0 and H == t["u"] and t["borrow2"] == 0,
                 "s1=q-1": lambda t, k, H: H < q and t["s1"] == q - 1 and H == t["u"] + 1 and t["borrow2"] == 1,
                 "s1=1": lambda t, k, H: H < q and t["s1"] == 1 and t["borrow2"] == 0,
                 "H=0": lambda t, k, H: H == 0 and t["s1"] == t["u"] and t["borrow2"] == 0,
                 "H=q-1 u=0": lambda t, k, H: H == q - 1 and t["u"] == 0 and t["s1"] == 1 and t["borrow2"] == 1},
        "hge": {"H=q u=0": lambda t, k, H: H == q and t["u"] == 0 and t["s1"] == 0,
                "H=q+c u=c": lambda t, k, H: q < H < W - 1 and t["u"] == H - q and t["s1"] == 0,
                "H=q+c u=c+1": lambda t, k, H: q < H < W - 1 and t["u"] == H - q + 1 and t["s1"] == 1,
                "H=W-1 u=cq-1": lambda t, k, H: H == W - 1 and t["u"] == cq - 1 and t["s1"] == 0,
                "H=W-1 u=cq": lambda t, k, H: H == W - 1 and t["u"] == cq and t["s1"] == 1},
        "wrap": {"H=W-1 u=0": lambda t, k, H: H == W - 1 and t["u"] == 0 and t["s1"] == q + 1,
                 "H=W-1 u=cq-2": lambda t, k, H: H == W - 1 and t["u"] == cq - 2 and t["s1"] == W - 1,
                 "H=q+1 u=0": lambda t, k, H: H == q + 1 and t["u"] == 0 and t["s1"] == W - 1},
    }


@pytest.mark.parametrize("l", T.LEVELS)
def test_every_record_is_what_its_kind_and_name_say(fx, l):
    q = T.curve_q(l)
    W = 1 << (2 * l)
    assert q >> (2 * l - 1) == 1 and pow(2, q - 1, q) == 1
    claims = _claims(l, q)
    seen = set()
    for c in fx.of(l):
        what = (c["kind"], c["name"])
        assert what not in seen
        seen.add(what)
        assert (len(c["priv"]), len(c["k"]), len(c["hash"]), len(c["sig"]), len(c["pub"])) == (l // 4, l // 4, l // 4, 3 * l // 8, l // 2), what
        d, k, H = T.le(c["priv"]), T.le(c["k"]), T.le(c["hash"])
        assert 0 < d < q and 0 < k < q, what
        t = T.record_tail(c, q)
        assert 0 < t["r"] < q and t["u"] == (k - t["r"]) % q, what
        assert T.le(c["sig"][l // 8:]) == t["s1"], what                       # the reference's octets ARE the model's
        m = re.fullmatch(r"top=(\d) t2=(\d) sub=(\d)", c["name"])
        if m:
            assert c["kind"] == "fold" and t["event"] == tuple(int(x) for x in m.groups()), what
        else:
            assert claims[c["kind"]][c["name"]](t, k, H), (what, t)
        if c["kind"] == "wrap":
            # the raw H went into zzSubMod: u < H - q, the borrow added q once, and what came out is no residue
            assert H >= q and t["u"] < H - q and t["borrow2"] == 1 and q <= t["s1"] == t["u"] - H + q + W, what
            assert c["verify"] == ERR_BAD_SIG != 0, what
        else:
            assert t["s1"] == (k - t["r"] - H) % q < q and c["verify"] == 0, what
            if c["kind"] == "hge":
                assert H >= q and t["u"] >= H - q and t["borrow2"] == 1, what
            elif c["kind"] in ("sub1", "sub2"):
                assert H < q, what
    for kind in T.KINDS:                                                        # every promised case is there, under both OIDs
        assert set(claims[kind]) <= {n for k_, n in seen if k_ == kind}, kind
        oids = {len(c["oid"]) % 4 for c in fx.of(l, kind)}
        assert len(fx.of(l, kind)) >= 2 and len(oids) == 2, kind
    from bee2_amd.engine import LEVEL_OID
    assert {c["oid"] for c in fx.of(l)} >= {bytes(LEVEL_OID[l])} and len({c["oid"] for c in fx.of(l)}) == 2


@pytest.mark.parametrize("l", T.LEVELS)
def test_the_bound_on_the_first_fold_and_what_it_leaves_reachable(l):
    """signtail.reachable against the passes themselves: at every edge of every range of r, for every m the bound allows, the
    passes of mod_q_ct on v = r + m q give an event of the reachable set, inside that event's range; the events outside are ruled
    out with a stated reason.  l = 128 and 256: the first fold stays below 2 q, so t2 = 1 cannot occur; l = 192: below 5 q."""
    q = T.curve_q(l)
    W = 1 << (2 * l)
    cq = W - q
    hi_max, v_max, m_max = T.fold_bound(l, q)
    assert hi_max == (((1 << l) - 1) + (1 << l)) * (q - 1) >> (2 * l) and v_max == W - 1 + hi_max * cq
    assert m_max == {128: 1, 192: 4, 256: 1}[l] and (m_max + 1) * q > v_max
    R = T.reachable(l, q)
    for e in T.all_events():
        assert (e in R) != isinstance(T.event_range(l, q, e), str)
    assert (any(t2 for _, t2, _ in R)) == (l == 192)
    assert {top for top, _, _ in R} == set(range(m_max + 1))
    hit = set()
    for m in range(m_max + 1):
        edges = {1, 2, cq - 1, cq, cq + 1, q - 2, q - 1, v_max - m * q - 1, v_max - m * q}
        for j in range(m_max + 2):
            edges |= {j * cq - 1, j * cq, j * cq + 1}
        for r in sorted(edges):
            if 0 < r < q and r + m * q <= v_max:
                e, got = T.fold_passes(l, q, r + m * q)
                assert got == r and e in R and R[e][0] <= r <= R[e][1] and sum(e) == m, (m, hex(r), e)
                hit.add(e)
    assert hit == set(R)
    for e, (lo, hi) in R.items():                                               # ... and the ranges are tight at both ends
        m = sum(e)
        assert T.fold_passes(l, q, lo + m * q)[0] == e and T.fold_passes(l, q, hi + m * q)[0] == e
        for r in (lo - 1, hi + 1):
            if 0 < r < q and r + m * q <= v_max:
                assert T.fold_passes(l, q, r + m * q)[0] != e


@pytest.mark.parametrize("l", T.LEVELS)
def test_the_fixture_witnesses_exactly_the_reachable_events(fx, l):
    """coverage is a condition: losing the record of any reachable event fails here"""
    q = T.curve_q(l)
    seen = {}
    for c in fx.of(l):
        seen.setdefault(T.record_tail(c, q)["event"], []).append(c["name"])
    R = T.reachable(l, q)
    assert set(seen) == set(R), (sorted(set(R) - set(seen)), sorted(set(seen) - set(R)))
    for e in R:                                                                 # each by a record that names it, too
        assert "top=%d t2=%d sub=%d" % e in seen[e], e
    # with and without the final subtraction at every top limb that allows both; t2 = 1 at every top limb it can occur with
    for top in {t for t, _, _ in R}:
        assert {(top, 0, s) in seen for s in (0, 1) if (top, 0, s) in R} == {True}
    if l == 192:
        assert {e[0] for e in seen if e[1]} == {1, 2, 3}


@pytest.mark.parametrize("l", T.LEVELS)
def test_the_oracle_gives_every_record(fx, orc, l):
    """oracle/bign_oracle.c restates zzMod and zzSubMod with H fed in as it is: signature, public key and verdict of every record"""
    for c in fx.of(l):
        what = (c["kind"], c["name"])
        assert orc.sign_rnd(l, c["oid"], c["hash"], c["priv"], c["k"]) == (0, c["sig"], 1), what
        assert orc.pubkey_calc(l, c["priv"]) == (0, c["pub"]), what
        assert orc.verify_l(l, c["oid"], c["hash"], c["sig"], c["pub"]) == c["verify"], what


@pytest.mark.skipif(not refgen.have_ref(), reason="oracle/_ref not built")
def test_the_generator_writes_the_committed_file(tmp_path, capsys):
    import make_golden_sign_tail
    out = tmp_path / "bign_sign_tail.json"
    make_golden_sign_tail.main(str(out))
    capsys.readouterr()
    assert out.read_bytes() == open(T.PATH, "rb").read()
    assert all(set(r) == {"l", "kind", "name", "oid", "priv", "k", "hash", "sig", "pub", "verify"} for r in json.load(open(T.PATH))["records"])
