"""-m gpu: the belt-dwp / belt-che record batch (bee2hip_beltAE_*_ragged*) against the C oracle, record by record, every
output octet compared (tests/beltaegrid.py builds the batches; tests/test_beltae.py pins the oracle to the reference).

The stream entry is a device-pointer batch entry that is not in the contract registry of tests/devcontract.py, so this file
holds it to the same contract itself, as tests/test_gpu_bashprg.py does: every buffer is a slice of one allocation filled with
a seeded pattern, at the weakest alignment the header grants, with 4 KiB of pattern on each side; after a call the outputs
are the oracle's over their whole range and every other octet of the allocation -- inputs and guards -- is what it was; in
place gives the out-of-place result; after one eager call the entry replays from a graph on fresh inputs, and scratch that
would have to grow refuses a capture."""
import json
import os
import random
import struct

import numpy as np
import pytest
import torch

import beltaegrid as G
import orclib
from bee2_amd import engine as E
from gpulib import engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096


class Arena:
    """named buffers inside one device allocation of seeded pattern, GUARD octets of it around each"""

    def __init__(self, seed):
        self.seed, self.at, self.data, self.pos = seed, {}, {}, GUARD

    def add(self, name, data, off=0):
        """`data` at an address = off mod 256 (a length: that many octets of pattern)"""
        start = (self.pos + 255) // 256 * 256 + off
        n = data if isinstance(data, int) else len(data)
        self.at[name], self.pos = (start, n), start + n + GUARD
        if not isinstance(data, int):
            self.data[name] = bytes(data)
        return self

    def build(self):
        self.image = np.frombuffer(random.Random(self.seed).randbytes(self.pos), dtype=np.uint8).copy()
        for name, d in self.data.items():
            self.put(name, d)
        self.dev = torch.from_numpy(self.image).cuda()
        assert self.dev.data_ptr() % 256 == 0
        return self

    def put(self, name, d):
        s, n = self.at[name]
        assert len(d) == n
        self.image[s:s + n] = np.frombuffer(bytes(d), dtype=np.uint8)

    def refill(self):
        self.dev.copy_(torch.from_numpy(self.image))
        torch.cuda.synchronize()

    def t(self, name):
        s, n = self.at[name]
        return self.dev[s:s + n]

    def fetch(self, outputs):
        """-> {name: bytes} of the outputs, after checking that nothing else changed"""
        torch.cuda.synchronize()
        got = self.dev.cpu().numpy()
        mask = np.ones(self.pos, dtype=bool)
        for name in outputs:
            s, n = self.at[name]
            mask[s:s + n] = False
        bad = np.nonzero((got != self.image) & mask)[0]
        assert bad.size == 0, f"{bad.size} octets outside the outputs changed, first at {int(bad[0])}: {self.at}"
        return {name: got[self.at[name][0]:self.at[name][0] + self.at[name][1]].tobytes() for name in outputs}


def _q(xs):
    return struct.pack(f"<{len(xs)}Q", *xs)


def _i(xs):
    return struct.pack(f"<{len(xs)}I", *xs)


def arena(b, unwrap, src, tags_in=None, inplace=True, shift=0, order=None, ivs=None, hblob=None, seed=1, headers=True):
    """the buffers of one call: src 16-aligned (the grid's offsets are start alignments), a separate dst at 256 k + shift,
    offsets at + 8, codes / order at + 4, ivs and tags at odd addresses, headers 16-aligned (the grid's header offsets are
    start alignments too)"""
    A = Arena(seed).add("src", src)
    if not inplace:
        A.add("dst", len(src), shift)
    A.add("ivs", b.ivs if ivs is None else ivs, 5).add("off", _q(b.offsets), 8)
    if headers:
        A.add("hdrs", b.hblob if hblob is None else hblob).add("hoff", _q(b.hoffsets), 8)
    A.add("tags", tags_in if unwrap else 8 * b.n, 1)
    if unwrap:
        A.add("codes", 4 * b.n, 4)
    if order is not None:
        A.add("order", _i(order), 4)
    return A.build()


def call(eng, b, A, unwrap):
    has = lambda k: A.t(k) if k in A.at else None
    eng.beltAE_ragged_stream(unwrap, b.mode, b.key, A.t("ivs"), has("hdrs"), has("hoff"), A.t("src"), A.t("off"),
                             A.t("dst") if "dst" in A.at else A.t("src"), A.t("tags"), b.n, codes=has("codes"), order=has("order"))


def outputs(A, unwrap):
    return (["dst"] if "dst" in A.at else ["src"]) + (["codes"] if unwrap else ["tags"])


def run(eng, b, unwrap, src, **kw):
    """-> (text out, tags out or None, codes or None); everything but the outputs is checked to be untouched"""
    A = arena(b, unwrap, src, **kw)
    call(eng, b, A, unwrap)
    got = A.fetch(outputs(A, unwrap))
    out = got.get("dst", got.get("src"))
    return out, got.get("tags"), list(struct.unpack(f"<{b.n}I", got["codes"])) if unwrap else None


def check(eng, b, order=None, shifts=(1,), headers=True):
    """wrap and unwrap of batch b in place and into a separate dst, against the oracle"""
    ct, tags = b.want()
    for kw in [dict(inplace=True)] + [dict(inplace=False, shift=s) for s in shifts]:
        out, t, _ = run(eng, b, False, b.blob, order=order, seed=2, headers=headers, **kw)
        assert out == ct and t == tags, ("wrap", kw)
        out, _, codes = run(eng, b, True, ct, tags_in=tags, order=order, seed=3, headers=headers, **kw)
        assert codes == [E.ERR_OK] * b.n and out == b.blob, ("unwrap", kw)


# ================================================================================================ vectors
@pytest.mark.parametrize("embed", [False, True], ids=["alone", "at-37-of-100"])
@pytest.mark.parametrize("name,mode", [("belt_dwp.json", 0), ("belt_che.json", 1)])
def test_standard_vectors_through_the_host_entries(name, mode, embed):
    """the standard's wrap and unwrap vectors of belt-dwp and belt-che (STB 34.101.31 annex A, the "kat" entries of
    tests/golden/belt_dwp.json and belt_che.json) through wrap and unwrap, as a batch of one and at index 37 of a
    batch of 100 whose other records are checked against the oracle"""
    eng, orc = engine(), orclib.load()
    kat = [k for k in json.load(open(os.path.join(ROOT, "tests", "golden", name)))["kat"] if k["op"] in ("wrap", "unwrap")]
    assert kat
    rnd = random.Random(37 + mode)
    n, at = (100, 37) if embed else (1, 0)
    for k in kat:
        key, iv, hdr, crit, out, mac = (bytes.fromhex(k[x]) for x in ("key", "iv", "open", "crit", "out", "mac"))
        pt, ct = (crit, out) if k["op"] == "wrap" else (out, crit)
        ivs = [rnd.randbytes(16) for _ in range(n)]
        hdrs = [rnd.randbytes(rnd.randrange(0, 60)) for _ in range(n)]
        texts = [rnd.randbytes(rnd.randrange(0, 200)) for _ in range(n)]
        ivs[at], hdrs[at], texts[at] = iv, hdr, pt
        code, cts, tags = eng.beltAE_wrap_ragged(mode, key, ivs, hdrs, texts)
        assert code == E.ERR_OK and cts[at] == ct and tags[at] == mac, k["name"]
        want = [orc.dwp_wrap(texts[i], hdrs[i], key, ivs[i], G.MODES[mode]) for i in range(n)]
        assert cts == [w[1] for w in want] and tags == [w[2] for w in want]
        code, pts, codes = eng.beltAE_unwrap_ragged(mode, key, ivs, hdrs, cts, tags)
        assert code == E.ERR_OK and codes == [E.ERR_OK] * n and pts == texts


# ================================================================================================ length x alignment grid
@pytest.mark.parametrize("mode", sorted(G.MODES))
def test_grid_every_length_at_every_alignment(mode):
    """text lengths 0 .. 49, 63 .. 65, 127 .. 129, 255 .. 257 at every start offset mod 16, headers of 0 / 1 / 15 / 16 / 17 / 33
    octets starting at 0 / 1 / 7 / 15 mod 16 (tests/test_beltae.py proves the coverage), wrap and unwrap.  In place, and into
    a separate dst at every alignment mod 4 other than the source's"""
    check(engine(), G.grid(mode), shifts=(1, 2, 3))


@pytest.mark.parametrize("key_len", G.KEY_LENS)
@pytest.mark.parametrize("mode", sorted(G.MODES))
def test_every_key_length(mode, key_len):
    check(engine(), G.edge(65, mode, key_len))


# ================================================================================================ batch edges
EDGE_N = (1, 63, 64, 65, 127, 128, 129, 1025)


@pytest.mark.parametrize("n", EDGE_N)
def test_batch_sizes_around_a_wavefront_and_the_bucketing_threshold(n):
    """partial wavefronts and workgroups, both sides of n = 128 (from there on the library buckets the lengths itself),
    records of 4095 / 4096 / 4097 / 6000 octets among short and empty ones; with the order omitted, with the caller's, and
    with the caller's reversed: the same result"""
    eng = engine()
    b = G.edge(n, EDGE_N.index(n) % 2, G.KEY_LENS[EDGE_N.index(n) % 3])
    check(eng, b)
    check(eng, b, order=b.order())
    ct, tags = b.want()
    out, t, _ = run(eng, b, False, b.blob, order=list(reversed(b.order())), seed=5)
    assert out == ct and t == tags


def test_empty_headers_by_null_pointers_and_a_batch_of_empty_records():
    eng = engine()
    for mode in G.MODES:
        blob, offsets = G.pack([0, 5, 0, 0, 300, 0, 16], 9)
        b = G.Batch(mode, bytes(range(24)), blob, offsets, [0] * 7, 9)
        check(eng, b, headers=False, shifts=(2,))
        e = G.Batch(mode, bytes(16), b"", [0] * 131, [0] * 130, 10)           # 130 records, all empty, no text at all
        ct, tags = e.want()
        assert ct == b"" and len(set(tags[8 * i:8 * i + 8] for i in range(130))) == 130          # (every record has its own iv)
        out, t, _ = run(eng, e, False, b"")
        assert t == tags
        _, _, codes = run(eng, e, True, b"", tags_in=tags, headers=False)
        assert codes == [E.ERR_OK] * 130


# ================================================================================================ the counter's carry
def test_dwp_counter_carries_out_of_its_low_word_inside_a_record():
    """the committed carry record (E_K(iv) mod 2^32 >= 2^32 - 2^12, 2^12 + 16 blocks: tests/test_beltae.py asserts it) beside
    200 short records"""
    eng = engine()
    c = json.load(open(os.path.join(ROOT, "tests", "golden", "belt_ae_ragged.json")))["carry"]
    x = G.carry_inputs(c["iv"])
    rnd = random.Random(0xCA)
    lens = [rnd.randrange(0, 100) for _ in range(201)]
    lens[77] = len(x["text"])
    blob, offsets = G.pack(lens, 12)
    blob = blob[:offsets[77]] + x["text"] + blob[offsets[78]:]
    hl = [rnd.randrange(0, 30) for _ in range(201)]
    hl[77] = len(x["hdr"])
    b = G.Batch(0, x["key"], blob, offsets, hl, 13)
    b.ivs = b.ivs[:16 * 77] + x["iv"] + b.ivs[16 * 78:]
    b.hblob = b.hblob[:b.hoffsets[77]] + x["hdr"] + b.hblob[b.hoffsets[78]:]
    ct, tags = b.want()
    assert tags[8 * 77:8 * 78].hex() == c["tag"] and G.sha(ct[offsets[77]:offsets[78]]) == c["ct_sha256"]
    check(eng, b)


# ================================================================================================ unwrap
@pytest.mark.parametrize("mode", sorted(G.MODES))
def test_unwrap_refuses_exactly_the_damaged_record(mode):
    """one bit flipped in a tag, a ciphertext, a header or an iv: that record gives ERR_BAD_MAC and zero plaintext, every other
    record -- the records of 1 .. 7 octets on both sides share dwords with it -- is intact and ERR_OK"""
    eng, orc = engine(), orclib.load()
    rnd = random.Random(0xBAD + mode)
    lens = [rnd.choice((1, 2, 3, 5, 7, 15, 16, 17, 33, 300)) for _ in range(70)]
    blob, offsets = G.pack(lens, 5)
    b = G.Batch(mode, rnd.randbytes(32), blob, offsets, [rnd.randrange(1, 40) for _ in lens], 6)
    ct, tags = b.want()

    def flipped(buf, pos, bit):
        x = bytearray(buf)
        x[pos] ^= 1 << bit
        return bytes(x)

    for k, what in enumerate(("tag", "ct", "hdr", "iv", "last octet", "tag last octet")):
        shared = [j for j in range(1, b.n - 1) if offsets[j] % 4 and offsets[j + 1] % 4]          # a neighbour on either side shares
        i = shared[(11 * k + 3) % len(shared)]                                                    # a dword with the refused record
        kw, src, tg = {}, ct, tags
        if what == "tag":
            tg = flipped(tags, 8 * i + rnd.randrange(7), rnd.randrange(8))
        elif what == "tag last octet":
            tg = flipped(tags, 8 * i + 7, 7)
        elif what == "ct":
            src = flipped(ct, offsets[i] + rnd.randrange(lens[i]), rnd.randrange(8))
        elif what == "last octet":
            src = flipped(ct, offsets[i + 1] - 1, 0)
        elif what == "hdr":
            kw["hblob"] = flipped(b.hblob, b.hoffsets[i] + rnd.randrange(b.hoffsets[i + 1] - b.hoffsets[i]), rnd.randrange(8))
        else:
            kw["ivs"] = flipped(b.ivs, 16 * i + rnd.randrange(16), rnd.randrange(8))
        want = bytearray(b.blob)
        want[offsets[i]:offsets[i + 1]] = bytes(lens[i])
        for inplace in (True, False):
            out, _, codes = run(eng, b, True, src, tags_in=tg, inplace=inplace, shift=3, seed=20 + k, **kw)
            assert codes == [E.ERR_BAD_MAC if j == i else E.ERR_OK for j in range(b.n)], what
            assert out == bytes(want), what
        code, _ = orc.dwp_unwrap(b.text(i, src), b.hdr(i, kw.get("hblob")), tg[8 * i:8 * i + 8], b.key, b.iv(i, kw.get("ivs")),
                                 G.MODES[mode])
        assert code == G.ERR_BAD_MAC


# ================================================================================================ host entries
@pytest.mark.parametrize("mode", sorted(G.MODES))
def test_host_entries_equal_the_stream_entry(mode):
    eng = engine()
    b = G.edge(129, mode, 24)
    ct, tags = b.want()
    texts, hdrs, ivs = ([f(i) for i in range(b.n)] for f in (b.text, b.hdr, b.iv))
    code, cts, tg = eng.beltAE_wrap_ragged(mode, b.key, ivs, hdrs, texts)
    assert code == E.ERR_OK and b"".join(cts) == ct and b"".join(tg) == tags
    out, t, _ = run(eng, b, False, b.blob)
    assert out == b"".join(cts) and t == b"".join(tg)
    bad = list(tg)
    bad[5] = bytes([bad[5][0] ^ 1]) + bad[5][1:]
    code, pts, codes = eng.beltAE_unwrap_ragged(mode, b.key, ivs, hdrs, cts, bad)
    assert code == E.ERR_OK and codes == [E.ERR_BAD_MAC if i == 5 else E.ERR_OK for i in range(b.n)]
    assert pts == [bytes(len(texts[i])) if i == 5 else texts[i] for i in range(b.n)]
    code, cts0, tg0 = eng.beltAE_wrap_ragged(mode, b.key, ivs, None, texts)          # NULL headers through the host entry
    nb = G.Batch(mode, b.key, b.blob, b.offsets, [0] * b.n, 1, ivs=b.ivs)
    assert code == E.ERR_OK and (b"".join(cts0), b"".join(tg0)) == nb.want()


# ================================================================================================ capture
def _fresh(b, seed):
    """a batch of the same shape with other contents"""
    rnd = random.Random(seed)
    return G.Batch(b.mode, b.key, rnd.randbytes(len(b.blob)), b.offsets, [b.hoffsets[i + 1] - b.hoffsets[i] for i in range(b.n)], seed)


@pytest.mark.parametrize("unwrap", [False, True], ids=["wrap", "unwrap"])
@pytest.mark.parametrize("mode", sorted(G.MODES))
def test_replays_from_a_graph_on_fresh_inputs(mode, unwrap):
    """one eager call at the size on a side stream, the same call captured (order given), replayed twice on refilled buffers"""
    eng = engine()
    b = G.edge(129, mode, 32)
    order = b.order()

    def fill(A, x):
        ct, tags = x.want()
        A.put("src", ct if unwrap else x.blob)
        A.put("ivs", x.ivs)
        A.put("hdrs", x.hblob)
        if unwrap:
            A.put("tags", tags)
        A.refill()

    def verify(A, x, what):
        ct, tags = x.want()
        got = A.fetch(outputs(A, unwrap))
        if unwrap:
            assert got["dst"] == x.blob and got["codes"] == bytes(4 * x.n), what
        else:
            assert got["dst"] == ct and got["tags"] == tags, what

    A = arena(b, unwrap, b.want()[0] if unwrap else b.blob, tags_in=b.want()[1], inplace=False, shift=1, order=order, seed=30)
    cap = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(cap):
        call(eng, b, A, unwrap)
    cap.synchronize()
    verify(A, b, "eager on a side stream")
    A.refill()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cap):
        call(eng, b, A, unwrap)
    for seed in (41, 42):
        x = _fresh(b, seed)
        fill(A, x)
        graph.replay()
        verify(A, x, f"replay {seed}")


def test_an_unprimed_order_refuses_the_capture():
    """without an order the library needs scratch of its own on this stream for the bucketing, which nothing has primed: an
    allocation under capture is refused before anything touches the stream (as for the bash-prg batch).  The batch is larger
    than any other test's on a stream of this priority, so whichever stream the pool hands out would have to grow"""
    eng = engine()
    b = G.edge(2051, 0, 16)
    A = arena(b, False, b.blob, inplace=False, shift=1, seed=50)
    cap = torch.cuda.Stream(priority=-1)
    marker = torch.zeros(64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.stream(cap):
        g2.capture_begin()
        try:
            marker.fill_(7)
            with pytest.raises(E.EngineError, match="capture"):
                call(eng, b, A, False)
        finally:
            g2.capture_end()
    torch.cuda.synchronize()
    assert int(marker.sum()) == 0
    g2.replay()
    torch.cuda.synchronize()
    assert int(marker.sum()) == 7 * 64
    assert A.fetch([]) == {}
    with torch.cuda.stream(cap):
        call(eng, b, A, False)                       # eagerly the scratch is made and the call works
    cap.synchronize()
    got = A.fetch(outputs(A, False))
    assert (got["dst"], got["tags"]) == b.want()
