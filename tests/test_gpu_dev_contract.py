"""-m gpu: what include/bee2hip.h and INTEGRATION.md promise about HOW the bee2hip_*_dev entries may be called, held for every
record of tests/devcontract.py:

 a. range and alignment -- every buffer is a slice of one allocation filled with a seeded pattern, at the weakest alignment the
    header grants (16-byte buffers at base + 16 / 48 / 112 / 240), with 4 KiB of pattern on each side.  After the call the
    outputs are the oracle's over their whole range, and every other byte of the allocation -- inputs, and the guards in front
    of and behind every buffer -- is what it was;
 b. aliasing -- in place where the header allows it gives the out-of-place result; ranges that overlap at any other distance
    are refused with ERR_BAD_INPUT before anything is launched;
 c. capture -- after one eager call every capturable entry replays from a hipGraph on fresh inputs; what cannot be captured
    (keyed verification, a one-signer key the cache does not hold, scratch that would have to grow) says so with an error before
    anything touches the capturing stream, and a key that becomes busy inside a capture is not promoted there.

Everything compared is bit-exact.  Only the belt-sde outputs are sampled (the oracle is quadratic per sector): first, last and
every ceil(n / 40)-th sector; guards and inputs are always compared in full."""
import zlib

import numpy as np
import pytest
import torch

import devcontract as dc
from bee2_amd import engine as E
from gpulib import engine, exp_engine

pytestmark = pytest.mark.gpu

# (collection also happens where there is no GPU: the named sizes only need the count when a test runs)
CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def _seed(*what):
    return zlib.crc32(repr(what).encode()) & 0xFFFF


def place(orc, case, off16, pattern_seed):
    """the case's buffers inside one device allocation -> (layout, image on entry, allocation, {name: slice})"""
    lay = dc.Layout(case, off16)
    img = lay.image(case, pattern_seed, orc)
    arena = torch.empty(lay.total, dtype=torch.uint8, device="cuda")
    assert arena.data_ptr() % 256 == 0
    refill(arena, img)
    T = {b.name: arena[lay.at[b.name][0]: lay.at[b.name][0] + lay.at[b.name][1]] for b in case.bufs}
    for b in case.bufs:
        assert not len(b.data) or T[b.name].data_ptr() % 256 == (off16 if b.align == 16 else b.align)
    return lay, img, arena, T


def refill(arena, img):
    arena.copy_(torch.from_numpy(img))
    torch.cuda.synchronize()


def check(lay, case, img, arena, want, what):
    got = arena.cpu().numpy()
    exp, mask = lay.expected(case, img, want)
    bad = np.nonzero((got != exp) & mask)[0]
    assert bad.size == 0, (f"{what}: {bad.size} bytes differ from {lay.where(int(bad[0]))} to {lay.where(int(bad[-1]))}: "
                           f"got {got[bad[:8]].tolist()} want {exp[bad[:8]].tolist()}")


# ======================================================================================================== a. range and alignment
CASES = [(r, s) for r in dc.REGISTRY for s in r.sizes]


@pytest.mark.parametrize("rec,size", CASES, ids=[f"{r.name}-{dc.size_id(s)}" for r, s in CASES])
def test_outputs_in_range_inputs_and_guards_untouched_at_the_granted_alignment(orc, rec, size):
    eng = engine()
    size = dc.resolve(size, CUS)
    case = rec.make(orc, size, _seed(rec.name, size))
    want = rec.expect(orc, case)
    offs = dc.OFFSETS16 if any(b.align == 16 for b in case.bufs) else dc.OFFSETS16[:1]
    for off in offs:
        lay, img, arena, T = place(orc, case, off, 0xA000 + off)
        rec.call(eng, T, case)
        torch.cuda.synchronize()
        check(lay, case, img, arena, want, f"{rec.name} size {size} at base + {off}")


# ======================================================================================================== b. aliasing
IN_PLACE = ("ecb_e", "ecb_d", "bde_e", "bde_d", "che")
NO_OVERLAP = IN_PLACE + ("cbc_d",)


def _call_src_dst(eng, rec, case, src, dst, s_out):
    T = {"src": src, "dst": dst}
    if s_out is not None:
        T["s_out"] = s_out
    rec.call(eng, T, case)


@pytest.mark.parametrize("nblocks", [2, 1025])
@pytest.mark.parametrize("name", IN_PLACE)
def test_in_place_gives_the_out_of_place_result(orc, name, nblocks):
    eng = engine()
    rec = dc.BY_NAME[name]
    case = rec.make(orc, nblocks, _seed(name, nblocks, "in place"))
    want = rec.expect(orc, case)
    # the same call with dst = src: one buffer, read and written
    one = dc.Case([dc.Buf("src", case["src"], 16, True)] + [dc.Buf(b.name, b.data, b.align, True) for b in case.bufs if b.name == "s_out"],
                  **case.args)
    want_one = {("src" if k == "dst" else k): v for k, v in want.items()}
    for off in dc.OFFSETS16[:2]:
        lay, img, arena, T = place(orc, one, off, 0xB000 + off)
        _call_src_dst(eng, rec, case, T["src"], T["src"], T.get("s_out"))
        torch.cuda.synchronize()
        check(lay, one, img, arena, want_one, f"{name} in place, {nblocks} blocks at base + {off}")


@pytest.mark.parametrize("nblocks", [2, 1025])
@pytest.mark.parametrize("name", NO_OVERLAP)
def test_overlapping_ranges_are_refused_and_nothing_runs(orc, name, nblocks):
    """dst = src +- 16 k with the ranges overlapping: ERR_BAD_INPUT, source, guards and the state output untouched, and a correct
    call right after works (the kernels' pointers are __restrict__: such a call used to return wrong bytes with ERR_OK)"""
    eng = engine()
    rec = dc.BY_NAME[name]
    case = rec.make(orc, nblocks, _seed(name, nblocks, "overlap"))
    nb = 16 * nblocks
    has_state = any(b.name == "s_out" for b in case.bufs)
    for k in sorted({1, 64, nblocks - 1}):
        if k >= nblocks:
            continue                                           # (no overlap left at this distance)
        for sign in (+1, -1):
            total = 2 * dc.GUARD + 512 + nb + 16 * k
            img = np.empty(total, dtype=np.uint8)
            orc.fill_np(img, 0xC000 + k)
            lo = dc.GUARD + 16                                  # (16-aligned and no more)
            s_at, d_at = (lo, lo + 16 * k) if sign > 0 else (lo + 16 * k, lo)
            img[s_at:s_at + nb] = np.frombuffer(case["src"], dtype=np.uint8)
            arena = torch.from_numpy(img).cuda()
            s_out = torch.from_numpy(img[:16].copy()).cuda() if has_state else None
            with pytest.raises(E.EngineError, match="err 109"):
                _call_src_dst(eng, rec, case, arena[s_at:s_at + nb], arena[d_at:d_at + nb], s_out)
            torch.cuda.synchronize()
            assert np.array_equal(arena.cpu().numpy(), img), (name, nblocks, k, sign)
            assert s_out is None or np.array_equal(s_out.cpu().numpy(), img[:16])
    if name == "cbc_d":                                        # in place stays refused for CBC decryption
        lay, img, arena, T = place(orc, case, 16, 0xC100)
        with pytest.raises(E.EngineError, match="err 109"):
            _call_src_dst(eng, rec, case, T["src"], T["src"], None)
        torch.cuda.synchronize()
        assert np.array_equal(arena.cpu().numpy(), img)
    # adjacent, disjoint ranges (dst right behind src, and right in front of it) are not overlap
    want = rec.expect(orc, case)
    for sign in (+1, -1):
        img = np.empty(2 * dc.GUARD + 512 + 2 * nb, dtype=np.uint8)
        orc.fill_np(img, 0xC200)
        lo = dc.GUARD + 16
        s_at, d_at = (lo, lo + nb) if sign > 0 else (lo + nb, lo)
        img[s_at:s_at + nb] = np.frombuffer(case["src"], dtype=np.uint8)
        arena = torch.from_numpy(img).cuda()
        _call_src_dst(eng, rec, case, arena[s_at:s_at + nb], arena[d_at:d_at + nb],
                      torch.zeros(16, dtype=torch.uint8, device="cuda") if has_state else None)
        torch.cuda.synchronize()
        exp = img.copy()
        exp[d_at:d_at + nb] = np.frombuffer(want["dst"], dtype=np.uint8)
        assert np.array_equal(arena.cpu().numpy(), exp), (name, nblocks, sign)
    # ... and the plain call still works
    lay, img, arena, T = place(orc, case, 16, 0xC300)
    rec.call(eng, T, case)
    torch.cuda.synchronize()
    check(lay, case, img, arena, want, f"{name} after the refusals")


# ======================================================================================================== c. capture
CAPTURABLE = [r for r in dc.REGISTRY if r.capture is not None]


def _same_args(a, b):
    return a.args.keys() == b.args.keys() and all(a.args[k] == b.args[k] for k in a.args)


@pytest.mark.parametrize("rec", CAPTURABLE, ids=[r.name for r in CAPTURABLE])
def test_entry_replays_from_a_hip_graph_on_fresh_inputs(orc, rec):
    """one eager call on a side stream (scratch, tables, dynamic-LDS grants), the same call captured, then replayed on the same
    buffers refilled from two fresh seeds -- inputs, output areas and guards alike -- and compared as in (a)"""
    eng = engine()
    size = dc.resolve(rec.capture, CUS)
    first = rec.make(orc, size, _seed(rec.name, "eager"))
    lay, img, arena, T = place(orc, first, 16, 0xD000)
    cap = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(cap):
        rec.call(eng, T, first)
    cap.synchronize()
    check(lay, first, img, arena, rec.expect(orc, first), f"{rec.name} eager on a side stream")
    refill(arena, img)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cap):
        rec.call(eng, T, first)
    for seed in (11, 12):
        case = rec.make(orc, size, _seed(rec.name, seed))
        assert _same_args(case, first) and [len(b.data) for b in case.bufs] == [len(b.data) for b in first.bufs]
        img = lay.image(case, 0xD100 + seed, orc)
        refill(arena, img)
        graph.replay()
        torch.cuda.synchronize()
        check(lay, case, img, arena, rec.expect(orc, case), f"{rec.name} replay {seed}")


def _fresh_stream():
    """a stream no earlier test has primed scratch on: torch hands its streams out of a small pool per priority, and only these
    tests take the high-priority ones"""
    return torch.cuda.Stream(priority=-1)


def _refused_inside_a_capture(stream, fn):
    """fn() raises an error that says "capture" while `stream` is capturing, and the capture is still good afterwards: it ends
    without an error and the one kernel of ours that went into it replays -- the refusal came before the library touched the stream"""
    marker = torch.zeros(64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        graph.capture_begin()
        try:
            marker.fill_(7)
            with pytest.raises(E.EngineError, match="capture"):
                fn()
        finally:
            graph.capture_end()
    torch.cuda.synchronize()
    assert int(marker.sum()) == 0
    graph.replay()
    torch.cuda.synchronize()
    assert int(marker.sum()) == 7 * 64


def test_keyed_verification_refuses_a_capture(orc):
    eng = engine()
    rec = dc.BY_NAME["verify_keyed_128"]
    assert rec.capture is None and "refused" in rec.why_not
    case = rec.make(orc, (257, 5), 3)
    lay, img, arena, T = place(orc, case, 16, 0xE000)
    st = _fresh_stream()
    with torch.cuda.stream(st):
        rec.call(eng, T, case)                       # eager: every key has its table, the stream its scratch
    st.synchronize()
    want = rec.expect(orc, case)
    check(lay, case, img, arena, want, "keyed, eager")
    refill(arena, img)
    _refused_inside_a_capture(st, lambda: rec.call(eng, T, case))
    assert np.array_equal(arena.cpu().numpy(), img)
    with torch.cuda.stream(st):
        rec.call(eng, T, case)                       # and eagerly it still works
    st.synchronize()
    check(lay, case, img, arena, want, "keyed, eager after the refusal")


def test_onekey_with_a_key_off_the_curve_refuses_a_capture(orc):
    """such a key is never cached (it takes the general path with the key repeated, through an upload and a synchronise): every
    call misses the key-table cache, and a miss under capture is refused"""
    eng = engine()
    case = dc.onekey_case(orc, 128, 257, 5)
    pub = bytearray(case.args["pubkey"])
    pub[3] ^= 0x20
    case.args["pubkey"] = bytes(pub)
    assert orc.pubkey_val(128, case.args["pubkey"]) == E.ERR_BAD_PUBKEY
    lay, img, arena, T = place(orc, case, 16, 0xE100)
    st = _fresh_stream()
    with torch.cuda.stream(st):
        dc.onekey_call(eng, T, case)
    st.synchronize()
    want = dc.onekey_expect(orc, case)
    check(lay, case, img, arena, want, "one signer, key off the curve, eager")
    refill(arena, img)
    _refused_inside_a_capture(st, lambda: dc.onekey_call(eng, T, case))
    assert np.array_equal(arena.cpu().numpy(), img)


@pytest.mark.parametrize("name,small", [("bde_e", 1024), ("verifyL_128", 256)])
def test_scratch_that_would_have_to_grow_refuses_a_capture(orc, name, small):
    """INTEGRATION: "call once eagerly with the largest size first".  A captured call at four times the size the eager call primed
    needs a bigger scratch block -- an allocation and a synchronise on the capturing stream; it is refused instead"""
    eng = engine()
    rec = dc.BY_NAME[name]
    st = _fresh_stream()
    case = rec.make(orc, small, 1)
    lay, img, arena, T = place(orc, case, 16, 0xE200)
    with torch.cuda.stream(st):
        rec.call(eng, T, case)
    st.synchronize()
    check(lay, case, img, arena, rec.expect(orc, case), f"{name} eager")
    big = rec.make(orc, 4 * small, 2)
    lay, img, arena, T = place(orc, big, 16, 0xE300)
    _refused_inside_a_capture(st, lambda: rec.call(eng, T, big))
    assert np.array_equal(arena.cpu().numpy(), img)
    with torch.cuda.stream(st):
        rec.call(eng, T, big)                        # eagerly the scratch grows and the call works
    st.synchronize()
    check(lay, big, img, arena, rec.expect(orc, big), f"{name} eager at four times the size")
    refill(arena, img)
    graph = torch.cuda.CUDAGraph()                   # ... and now that size can be captured
    with torch.cuda.graph(graph, stream=st):
        rec.call(eng, T, big)
    graph.replay()
    torch.cuda.synchronize()
    check(lay, big, img, arena, rec.expect(orc, big), f"{name} replayed at four times the size")


def test_a_key_that_becomes_busy_inside_a_capture_is_not_promoted_there(orc):
    """the flow the library's own message recommends -- a small eager call under the key, then a big batch captured -- crosses the
    16-bit-table threshold inside the capture (here 2^10 signatures, experiments library): the captured call must run on the tables
    the key has, build nothing, and not count; the next eager call promotes the key and gives the same verdicts"""
    eng = exp_engine()
    tune, stat = eng.lib.bee2hip_internal_tune, eng.lib.bee2hip_internal_stat
    l, small, big = 128, 256, 4096
    key, other = 0x2C01, 0x2C02
    cap = torch.cuda.Stream()
    try:
        assert tune(20, 10) == 0
        # the stream's scratch at the big size, under ANOTHER key (the captured call must not have to grow it)
        prime = dc.onekey_case(orc, l, big, 1, keyseed=other)
        lay, img, arena, T = place(orc, prime, 16, 0xF000)
        with torch.cuda.stream(cap):
            dc.onekey_call(eng, T, prime)
        cap.synchronize()
        check(lay, prime, img, arena, dc.onekey_expect(orc, prime), "priming call")
        first = dc.onekey_case(orc, l, small, 2, keyseed=key)
        lay_s, img_s, arena_s, T_s = place(orc, first, 16, 0xF100)
        with torch.cuda.stream(cap):
            dc.onekey_call(eng, T_s, first)          # the key's 8-bit table; 256 of the 1024 signatures towards the 16-bit one
        cap.synchronize()
        check(lay_s, first, img_s, arena_s, dc.onekey_expect(orc, first), "small eager call")
        live, builds = stat(5), stat(3)
        case = dc.onekey_case(orc, l, big, 3, keyseed=key)
        img = lay.image(case, 0xF200, orc)
        refill(arena, img)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=cap):
            dc.onekey_call(eng, T, case)
        assert (stat(5), stat(3)) == (live, builds), "a key table was built inside the capture"
        verdicts = None
        for seed in (21, 22):
            case = dc.onekey_case(orc, l, big, seed, keyseed=key)
            img = lay.image(case, 0xF200 + seed, orc)
            refill(arena, img)
            graph.replay()
            torch.cuda.synchronize()
            verdicts = dc.onekey_expect(orc, case)
            assert len(set(verdicts["codes"])) > 1               # (damaged entries among them)
            check(lay, case, img, arena, verdicts, f"replay {seed}")
        # the captured call did not count: 256 + 256 signatures are still below the threshold
        refill(arena_s, img_s)
        with torch.cuda.stream(cap):
            dc.onekey_call(eng, T_s, first)
        cap.synchronize()
        assert stat(5) == live
        # an eager call with the big batch promotes the key; same verdicts from the 16-bit table
        refill(arena, img)
        with torch.cuda.stream(cap):
            dc.onekey_call(eng, T, case)
        cap.synchronize()
        assert stat(5) == live + 1 and stat(3) == builds
        check(lay, case, img, arena, verdicts, "eager call that promotes the key")
        refill(arena, img)
        with torch.cuda.stream(cap):
            dc.onekey_call(eng, T, case)             # ... and on it
        cap.synchronize()
        check(lay, case, img, arena, verdicts, "eager call on the 16-bit table")
    finally:
        tune(20, -1)
