"""-m gpu: the bash-prg batch entries (bee2hip_bashPrgHash_ragged*, bee2hip_bashPrgAE_*_ragged*) against the Python model of
tests/orc_bashprg.py, every output octet compared.

The stream entries are device-pointer batch entries that the contract registry of tests/devcontract.py cannot describe (its
expected bytes come from the C oracle, which has no bash-prg), so this file holds them to the same contract itself: every
buffer is a slice of one allocation filled with a seeded pattern, at the weakest alignment the header grants, with 4 KiB of
pattern on each side; after a call the outputs are the model's over their whole range and every other octet of the allocation
-- inputs and guards -- is what it was; in place gives the out-of-place result; after one eager call the entry replays
from a graph on fresh inputs, and scratch that would have to grow refuses a capture."""
import json
import os
import random
import struct

import numpy as np
import pytest
import torch

import bashprggrid as G
import orc_bashprg as M
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


def ae_arena(b, unwrap, src, tags_in=None, inplace=True, shift=0, order=None, anns=None, hblob=None, seed=1, headers=True):
    """the buffers of one prg-ae call: src 16-aligned (the grid's offsets are start alignments), a separate dst at
    256 k + shift, offsets at + 8, announcements / codes / order at + 4, headers and tags at odd addresses"""
    A = Arena(seed).add("src", src)
    if not inplace:
        A.add("dst", len(src), shift)
    A.add("anns", b.anns if anns is None else anns, 4).add("off", _q(b.offsets), 8)
    if headers:
        A.add("hdrs", b.hblob if hblob is None else hblob, 3).add("hoff", _q(b.hoffsets), 8)
    A.add("tags", tags_in if unwrap else b.n * b.tag_len, 1)
    if unwrap:
        A.add("codes", 4 * b.n, 4)
    if order is not None:
        A.add("order", _i(order), 4)
    return A.build()


def ae_call(eng, b, A, unwrap):
    has = lambda k: A.t(k) if k in A.at else None
    eng.bashPrgAE_ragged_stream(unwrap, b.l, b.d, b.key, A.t("anns"), b.ann_len, has("hdrs"), has("hoff"), A.t("src"),
                                A.t("off"), A.t("dst") if "dst" in A.at else A.t("src"), A.t("tags"), b.tag_len, b.n,
                                codes=has("codes"), order=has("order"))


def ae_outputs(A, unwrap):
    return (["dst"] if "dst" in A.at else ["src"]) + (["codes"] if unwrap else ["tags"])


def run_ae(eng, b, unwrap, src, **kw):
    """-> (text out, tags out or None, codes or None)"""
    A = ae_arena(b, unwrap, src, **kw)
    ae_call(eng, b, A, unwrap)
    got = A.fetch(ae_outputs(A, unwrap))
    out = got.get("dst", got.get("src"))
    return out, got.get("tags"), list(struct.unpack(f"<{b.n}I", got["codes"])) if unwrap else None


def check_ae(eng, b, order=None, shifts=(1,)):
    """wrap and unwrap of batch b in place and into a separate dst, against the model"""
    ct, tags = b.want()
    for kw in [dict(inplace=True)] + [dict(inplace=False, shift=s) for s in shifts]:
        out, t, _ = run_ae(eng, b, False, b.blob, order=order, seed=2, **kw)
        assert out == ct and t == tags, ("wrap", kw)
        out, _, codes = run_ae(eng, b, True, ct, tags_in=tags, order=order, seed=3, **kw)
        assert codes == [E.ERR_OK] * b.n and out == b.blob, ("unwrap", kw)


def run_hash(eng, b, order=None, seed=4):
    A = Arena(seed).add("data", b.blob).add("off", _q(b.offsets), 8).add("out", b.n * b.out_len, 1)
    if order is not None:
        A.add("order", _i(order), 4)
    A.build()
    eng.bashPrgHash_ragged_stream(b.l, b.d, b.ann, A.t("data"), A.t("off"), A.t("out"), b.out_len, b.n,
                                  order=A.t("order") if order is not None else None)
    return A.fetch(["out"])["out"]


# ================================================================================================ vectors
@pytest.fixture(scope="module")
def fixtures():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "bash_prg.json")))


@pytest.mark.parametrize("embed", [False, True], ids=["alone", "at-37-of-100"])
def test_standard_vectors_through_the_host_entries(fixtures, embed):
    """A.5.1 - A.5.7 through bashPrgHash_ragged, A.6 through wrap and unwrap, as a batch of one and at index 37 of a batch
    of 100 whose other records are checked against the model"""
    eng = engine()
    rnd = random.Random(37)
    n, at = (100, 37) if embed else (1, 0)
    for v in fixtures["vectors"]:
        l, d = v["l"], v["d"]
        if v["kind"] == "hash":
            msgs = [rnd.randbytes(rnd.randrange(0, 300)) for _ in range(n)]
            msgs[at] = bytes.fromhex(v["msg"])
            code, outs = eng.bashPrgHash_ragged(l, d, bytes.fromhex(v["ann"]), msgs, v["out_len"])
            assert code == E.ERR_OK and outs[at].hex() == v["out"], v["name"]
            assert outs == [M.prg_hash(l, d, b"", m, v["out_len"]) for m in msgs]
            continue
        key, ann, hdr, text = (bytes.fromhex(v[k]) for k in ("key", "ann", "hdr", "text"))
        anns = [rnd.randbytes(len(ann)) for _ in range(n)]
        hdrs = [rnd.randbytes(rnd.randrange(0, 200)) for _ in range(n)]
        texts = [rnd.randbytes(rnd.randrange(0, 400)) for _ in range(n)]
        anns[at], hdrs[at], texts[at] = ann, hdr, text
        code, cts, tags = eng.bashPrgAE_wrap_ragged(l, d, key, anns, hdrs, texts, v["tag_len"])
        assert code == E.ERR_OK and cts[at].hex() == v["ct"] and tags[at].hex() == v["tag"]
        want = [M.ae_wrap(l, d, key, anns[i], hdrs[i], texts[i], v["tag_len"]) for i in range(n)]
        assert cts == [w[0] for w in want] and tags == [w[1] for w in want]
        code, pts, codes = eng.bashPrgAE_unwrap_ragged(l, d, key, anns, hdrs, cts, tags)
        assert code == E.ERR_OK and codes == [E.ERR_OK] * n and pts == texts


# ================================================================================================ length x alignment grid
@pytest.mark.parametrize("c", range(4))
@pytest.mark.parametrize("l,d", M.LD)
def test_ae_grid_every_length_at_every_alignment(l, d, c):
    """text lengths 0 .. r+17, 2r-1 .. 2r+1, 3r-16 .. 3r+1 at every start offset mod 16 (tests/test_bashprg.py proves the
    coverage), headers 0 / 1 / r-1 / r / r+1; configuration c sets the announcement, key and tag lengths.  In place, and into a
    separate dst at every alignment mod 4 other than the source's"""
    check_ae(engine(), G.ae_grid(l, d, c), shifts=(1, 2, 3))


@pytest.mark.parametrize("c", range(4))
@pytest.mark.parametrize("l,d", M.LD)
def test_hash_grid_every_length_at_every_alignment(l, d, c):
    b = G.hash_grid(l, d, c)
    assert run_hash(engine(), b) == b.want()


@pytest.mark.parametrize("l,d", M.LD)
def test_every_key_and_announcement_length(l, d):
    """key_len = l/8 .. 60 in steps of 4 with every announcement length: the start state is ann || key from octet 1 on"""
    eng = engine()
    r = M.rate(l, d, True)
    rnd = random.Random(l + d)
    for key_len in G.key_lens(l):
        for ann_len in G.ANN_LENS:
            lens = [rnd.choice((0, 1, 5, r - 1, r, r + 1, 200)) for _ in range(9)]
            blob, offsets = G.pack(lens, key_len * 64 + ann_len)
            b = G.AEBatch(l, d, rnd.randbytes(key_len), ann_len, 16, blob, offsets, [rnd.randrange(0, 40) for _ in lens], key_len + ann_len)
            ct, tags = b.want()
            out, t, _ = run_ae(eng, b, False, b.blob)
            assert out == ct and t == tags, (key_len, ann_len)
    for ann_len in G.ANN_LENS:
        blob, offsets = G.pack([rnd.randrange(0, 300) for _ in range(9)], ann_len)
        hb = G.HashBatch(l, d, rnd.randbytes(ann_len), 24, blob, offsets)
        assert run_hash(eng, hb) == hb.want(), ann_len


# ================================================================================================ batch edges
EDGE_N = (1, 63, 64, 65, 127, 128, 129, 1100)


@pytest.mark.parametrize("n", EDGE_N)
def test_batch_sizes_around_a_wavefront_and_the_bucketing_threshold(n):
    """partial wavefronts, both sides of n = 128 (from there on the library buckets the lengths itself), records of 4095 /
    4096 / 4097 / 20 000 octets among short and empty ones; with the order omitted and with the caller's"""
    eng = engine()
    l, d = M.LD[EDGE_N.index(n) % 6]
    b = G.ae_edge(n, l, d)
    check_ae(eng, b)
    check_ae(eng, b, order=b.order())
    h = G.hash_edge(n, l, d)
    assert run_hash(eng, h) == h.want()
    assert run_hash(eng, h, order=h.order()) == h.want()
    assert run_hash(eng, h, order=list(reversed(h.order()))) == h.want()


def test_empty_headers_by_null_pointers_and_a_batch_of_empty_records():
    eng = engine()
    blob, offsets = G.pack([0, 5, 0, 0, 300, 0], 9)
    b = G.AEBatch(192, 1, bytes(range(24)), 4, 8, blob, offsets, [0] * 6, 9)
    ct, tags = b.want()
    out, t, _ = run_ae(eng, b, False, b.blob, headers=False)
    assert out == ct and t == tags
    out, _, codes = run_ae(eng, b, True, ct, tags_in=tags, headers=False, inplace=False, shift=2)
    assert out == b.blob and codes == [0] * 6
    e = G.AEBatch(128, 2, bytes(16), 0, 64, b"", [0] * 131, [0] * 130, 10)           # 130 records, all empty, no text at all
    ct, tags = e.want()
    assert ct == b"" and len(set(tags[64 * i:64 * i + 64] for i in range(130))) == 1
    out, t, _ = run_ae(eng, e, False, b"")
    assert t == tags


# ================================================================================================ unwrap
def test_unwrap_refuses_exactly_the_damaged_record():
    """one bit flipped in a tag, a ciphertext, a header, an announcement or the last octet of a record: that record gives
    ERR_BAD_MAC and zero plaintext, every other record is intact and ERR_OK"""
    eng = engine()
    l, d = 256, 1
    r = M.rate(l, d, True)
    rnd = random.Random(0xBAD)
    lens = [rnd.choice((1, 7, r - 1, r, r + 1, 2 * r + 5, 300)) for _ in range(70)]
    blob, offsets = G.pack(lens, 5)
    b = G.AEBatch(l, d, rnd.randbytes(32), 16, 32, blob, offsets, [rnd.randrange(1, 2 * r) for _ in lens], 6)
    ct, tags = b.want()

    def flipped(buf, pos, bit):
        x = bytearray(buf)
        x[pos] ^= 1 << bit
        return bytes(x)

    for k, what in enumerate(("tag", "ct", "hdr", "ann", "last octet", "tag last octet")):
        i = (11 * k + 3) % b.n
        kw, src, tg = {}, ct, tags
        if what == "tag":
            tg = flipped(tags, i * b.tag_len + rnd.randrange(b.tag_len - 1), rnd.randrange(8))
        elif what == "tag last octet":
            tg = flipped(tags, i * b.tag_len + b.tag_len - 1, 7)
        elif what == "ct":
            src = flipped(ct, offsets[i] + rnd.randrange(lens[i]), rnd.randrange(8))
        elif what == "last octet":
            src = flipped(ct, offsets[i + 1] - 1, 0)
        elif what == "hdr":
            kw["hblob"] = flipped(b.hblob, b.hoffsets[i] + rnd.randrange(b.hoffsets[i + 1] - b.hoffsets[i]), rnd.randrange(8))
        else:
            kw["anns"] = flipped(b.anns, i * b.ann_len + rnd.randrange(b.ann_len), rnd.randrange(8))
        want = bytearray(b.blob)
        want[offsets[i]:offsets[i + 1]] = bytes(lens[i])
        for inplace in (True, False):
            out, _, codes = run_ae(eng, b, True, src, tags_in=tg, inplace=inplace, shift=3, seed=20 + k, **kw)
            assert codes == [E.ERR_BAD_MAC if j == i else E.ERR_OK for j in range(b.n)], what
            assert out == bytes(want), what
        code, want_pt = M.ae_unwrap(l, d, b.key, b.ann(i, kw.get("anns")), b.hdr(i, kw.get("hblob")), b.text(i, src),
                                    tg[i * b.tag_len:(i + 1) * b.tag_len])
        assert code == M.ERR_BAD_MAC and want_pt == bytes(lens[i])


# ================================================================================================ host entries
def test_host_entries_equal_the_stream_entries():
    eng = engine()
    b = G.ae_edge(129, 192, 2)
    ct, tags = b.want()
    texts, hdrs, anns = ([f(i) for i in range(b.n)] for f in (b.text, b.hdr, b.ann))
    code, cts, tg = eng.bashPrgAE_wrap_ragged(b.l, b.d, b.key, anns, hdrs, texts, b.tag_len)
    assert code == E.ERR_OK and b"".join(cts) == ct and b"".join(tg) == tags
    out, t, _ = run_ae(eng, b, False, b.blob)
    assert out == b"".join(cts) and t == b"".join(tg)
    bad = list(tg)
    bad[5] = bytes([bad[5][0] ^ 1]) + bad[5][1:]
    code, pts, codes = eng.bashPrgAE_unwrap_ragged(b.l, b.d, b.key, anns, hdrs, cts, bad)
    assert code == E.ERR_OK and codes == [E.ERR_BAD_MAC if i == 5 else E.ERR_OK for i in range(b.n)]
    assert pts == [bytes(len(texts[i])) if i == 5 else texts[i] for i in range(b.n)]
    h = G.hash_edge(129, 192, 2)
    code, outs = eng.bashPrgHash_ragged(h.l, h.d, h.ann, [h.msg(i) for i in range(h.n)], h.out_len)
    assert code == E.ERR_OK and b"".join(outs) == h.want() == run_hash(eng, h)


# ================================================================================================ capture
def _fresh(b, seed):
    """a batch of the same shape with other contents"""
    rnd = random.Random(seed)
    return G.AEBatch(b.l, b.d, b.key, b.ann_len, b.tag_len, rnd.randbytes(len(b.blob)), b.offsets,
                     [b.hoffsets[i + 1] - b.hoffsets[i] for i in range(b.n)], seed)


@pytest.mark.parametrize("unwrap", [False, True], ids=["wrap", "unwrap"])
def test_ae_replays_from_a_graph_on_fresh_inputs(unwrap):
    """one eager call at the size on a side stream, the same call captured (order given), replayed twice on refilled buffers"""
    eng = engine()
    b = G.ae_edge(129, 128, 1)
    order = b.order()

    def fill(A, x):
        ct, tags = x.want()
        A.put("src", ct if unwrap else x.blob)
        A.put("anns", x.anns)
        A.put("hdrs", x.hblob)
        if unwrap:
            A.put("tags", tags)
        A.refill()

    def check(A, x, what):
        ct, tags = x.want()
        got = A.fetch(ae_outputs(A, unwrap))
        if unwrap:
            assert got["dst"] == x.blob and got["codes"] == bytes(4 * x.n), what
        else:
            assert got["dst"] == ct and got["tags"] == tags, what

    A = ae_arena(b, unwrap, b.want()[0] if unwrap else b.blob, tags_in=b.want()[1], inplace=False, shift=1, order=order, seed=30)
    cap = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(cap):
        ae_call(eng, b, A, unwrap)
    cap.synchronize()
    check(A, b, "eager on a side stream")
    A.refill()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cap):
        ae_call(eng, b, A, unwrap)
    for seed in (41, 42):
        x = _fresh(b, seed)
        fill(A, x)
        graph.replay()
        check(A, x, f"replay {seed}")


def test_hash_replays_from_a_graph_and_an_unprimed_order_refuses_the_capture():
    eng = engine()
    h = G.hash_edge(129, 256, 2)
    order = h.order()
    A = Arena(50).add("data", h.blob).add("off", _q(h.offsets), 8).add("out", h.n * h.out_len, 1).add("order", _i(order), 4).build()
    call = lambda ordered: eng.bashPrgHash_ragged_stream(h.l, h.d, h.ann, A.t("data"), A.t("off"), A.t("out"), h.out_len, h.n,
                                                         order=A.t("order") if ordered else None)
    cap = torch.cuda.Stream(priority=-1)
    torch.cuda.synchronize()
    with torch.cuda.stream(cap):
        call(True)
    cap.synchronize()
    assert A.fetch(["out"])["out"] == h.want()
    A.refill()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cap):
        call(True)
    x = G.HashBatch(h.l, h.d, h.ann, h.out_len, random.Random(51).randbytes(len(h.blob)), h.offsets)
    A.put("data", x.blob)
    A.refill()
    graph.replay()
    assert A.fetch(["out"])["out"] == x.want()
    # without an order the library needs scratch for its own on this stream, which nothing has primed: an allocation under
    # capture is refused before anything touches the stream (as the registry's entries do)
    A.refill()
    marker = torch.zeros(64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.stream(cap):
        g2.capture_begin()
        try:
            marker.fill_(7)
            with pytest.raises(E.EngineError, match="capture"):
                call(False)
        finally:
            g2.capture_end()
    torch.cuda.synchronize()
    assert int(marker.sum()) == 0
    g2.replay()
    torch.cuda.synchronize()
    assert int(marker.sum()) == 7 * 64
    assert A.fetch([])  == {}
    with torch.cuda.stream(cap):
        call(False)                                  # eagerly the scratch is made and the call works
    cap.synchronize()
    assert A.fetch(["out"])["out"] == x.want()
