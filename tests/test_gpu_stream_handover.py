"""-m gpu: one drop-in stream whose steps are served by different engines (bee2_amd/csrc/staging.hpp with_host(): the host path of
host_small.hpp or a kernel, chosen per call).  Everything the next step needs travels through bee2's state struct, so a step on
one engine must leave the state exactly as the other engine would have.

The plans come from tests/streamplans.py (tests/test_stream_plans.py proves their coverage on the CPU).  Every step runs with the
path policy set for that step alone; the path counters are read before and after it and the state is copied after it.
  a. forced alternation: g c g c ..., c g c g ..., a seeded random pattern -- a hand-over at every size and for the serial kinds that
     auto mode never sends to the GPU.  Every output octet, every tag and digest in mid-stream against the oracle's own streaming
     functions (a tag in mid-stream: the oracle on the prefix).
  b. the state after every step of the alternating runs against an all-GPU and an all-host run of the same plan; for belt-ctr (and
     the counter inside a belt-dwp state) also against the oracle's 72-octet state, for belt-bde / belt-che the tweak s against the
     oracle's block loop.
  c. auto mode, as a caller gets it: per step the engine that streamplans predicts from its constants, and the one-shot calls with
     header, text and length block on different sides of their crossovers.
  d. the software fallback in mid-stream (the experiments build's injection hook: with_host() skips the device call and reports a
     failure; nothing faults on the device).

Masked in (b) -- scratch that no later Step reads, nothing else:
  belt_mac_st.block[filled .. 16)   the kernel walks every octet through block[] (mixed_kernels.hip:330-339), the host path takes
                                    whole blocks straight from the caller's buffer (host_small.hpp:218-225), so the octets BEHIND
                                    `filled` differ.  A later StepA writes block[filled++] before `filled` reaches 16 and absorbs the
                                    block only then (host_small.hpp:226-235); StepG overwrites [filled, 16) with the padding before
                                    it reads (host_small.hpp:246-248).  block[0 .. filled) and `filled` itself are compared."""
import ctypes
import struct

import pytest

import streamplans as SP
from gpulib import engine, exp_engine

pytestmark = pytest.mark.gpu

_sz = ctypes.c_size_t
POLICY = {"a": 0, "g": 1, "c": 2}
ERR_BAD_MAC = 511
KEY_LENS = (16, 24, 32)
_loaded = []                       # libraries whose policy this module has touched


@pytest.fixture(autouse=True)
def _auto_policy_on_every_exit():
    yield
    for L in _loaded:
        L.bee2hip_path_policy(0)


def _lib(exp=False):
    L = (exp_engine() if exp else engine()).lib
    if L not in _loaded:
        _loaded.append(L)
    L.bee2hip_path_policy(0)
    return L


def _counts(L):
    return tuple(L.bee2hip_path_count(i) for i in range(3))


def _key(orc, n):
    return orc.beltH()[128:128 + n]


def _iv(orc):
    return orc.beltH()[192:208]


# ------------------------------------------------------------------ the driver ---
class Run:
    """one stream: outs[k] = what step k returned (octets, a tag / digest, or a verdict), states[k] = the state blob after it,
    deltas[k] = how far the three path counters moved during it"""

    def __init__(self):
        self.outs, self.states, self.deltas = [], [], []


def _prefix(family):
    return "bashHash" if family in SP.BASH_LEVEL else {"CTR": "beltCTR", "DWP": "beltDWP", "CHE": "beltCHE", "MAC": "beltMAC",
                                                        "HASH": "beltHash"}.get(family, "belt" + family[:3])


def _start(L, family, key, iv):
    pre = _prefix(family)
    st = ctypes.create_string_buffer(getattr(L, pre + "_keep")())
    if family in SP.BASH_LEVEL:
        L.bashHashStart(st, _sz(SP.BASH_LEVEL[family]))
    elif family == "HASH":
        L.beltHashStart(st)
    elif family == "MAC" or family[:3] == "ECB":
        getattr(L, pre + "Start")(st, key, _sz(len(key)))
    else:
        getattr(L, pre + "Start")(st, key, _sz(len(key)), iv)
    return st


def _one_step(L, family, st, op, data, last_g, want):
    """-> what the step returned.  `want`: the expected tag, for a V step"""
    pre = _prefix(family)
    if op in "ED":
        buf = ctypes.create_string_buffer(data, len(data))
        getattr(L, pre + "Step" + op)(buf, _sz(len(data)), st)
        return buf.raw
    if op in "IAH":
        getattr(L, pre + "Step" + op)(data, _sz(len(data)), st)
        return None
    if family in ("DWP", "CHE"):
        if op == "V":
            return bool(getattr(L, pre + "StepV")(want, st))
        m = ctypes.create_string_buffer(8)
        getattr(L, pre + "StepG")(m, st)
        return m.raw
    if family == "MAC":                          # StepG in mid-stream, StepG2 / StepV2 (6 octets) at the end
        if op == "V":
            return bool(L.beltMACStepV2(want[:6], _sz(6), st))
        m = ctypes.create_string_buffer(8)
        if last_g:
            L.beltMACStepG2(m, _sz(6), st)
            return m.raw[:6]
        L.beltMACStepG(m, st)
        return m.raw
    if family == "HASH":                         # StepG in mid-stream, StepG2 (20 octets) at the end
        d = ctypes.create_string_buffer(32)
        if last_g:
            L.beltHashStepG2(d, _sz(20), st)
            return d.raw[:20]
        L.beltHashStepG(d, st)
        return d.raw
    n = SP.BASH_LEVEL[family] // 4
    d = ctypes.create_string_buffer(n)
    L.bashHashStepG(d, _sz(n), st)
    return d.raw


def run_plan(L, family, ops, pieces, key, iv, pat, wants, before_step=None):
    """pat: the policy of Start and of every step, len(ops) + 1 letters of 'g' (GPU), 'c' (host), 'a' (auto)"""
    assert len(pat) == len(ops) + 1
    run = Run()
    try:
        L.bee2hip_path_policy(POLICY[pat[0]])
        st = _start(L, family, key, iv)
        last_g = max((k for k, (op, _) in enumerate(ops) if op == "G"), default=-1)
        for k, (op, n) in enumerate(ops):
            if before_step:
                before_step(k)
            L.bee2hip_path_policy(POLICY[pat[k + 1]])
            c0 = _counts(L)
            run.outs.append(_one_step(L, family, st, op, pieces[k], k == last_g, wants[k]))
            c1 = _counts(L)
            run.deltas.append(tuple(b - a for a, b in zip(c0, c1)))
            run.states.append(st.raw)
    finally:
        L.bee2hip_path_policy(0)
    return run


# ------------------------------------------------------------- what the oracle says ---
def _pieces(orc, ops, seed):
    data = orc.fill(SP.total_bytes(ops), seed)
    out, off = [], 0
    for _, n in ops:
        out.append(data[off:off + n])
        off += n
    return out


def expected(orc, family, ops, pieces, key, iv):
    """per step: the octets an E / D step returns, the tag / digest of a G step, the tag a V step is given; None otherwise"""
    want = [None] * len(ops)
    msg = b"".join(pieces)
    last_g = max((k for k, (op, _) in enumerate(ops) if op == "G"), default=-1)
    if family in ("DWP", "CHE"):
        o_ops = [(op, p) if op in "EDIA" else ("G",) for (op, _), p in zip(ops, pieces)]
        out, macs = orc.dwp_steps(key, iv, o_ops, mode=family)
        off = 0
        for k, (op, n) in enumerate(ops):
            if op in "ED":
                want[k] = out[off:off + n]
                off += n
            elif op in "GV":
                want[k] = macs.pop(0)
        return want
    if family == "CTR":
        whole = orc.ctr(msg, key, iv, [n for _, n in ops])
    elif family[:3] == "ECB":
        code, whole = orc.ecb(msg, key, decr=family[-1] == "D")
        assert code == 0
    elif family[:3] == "CBC":
        code, whole = orc.cbc(msg, key, iv, decr=family[-1] == "D")
        assert code == 0
    elif family[:3] == "BDE":
        code, whole = orc.bde(msg, key, iv, decr=family[-1] == "D")
        assert code == 0
    else:
        off = 0
        for k, (op, n) in enumerate(ops):
            off += n
            if op in "GV":
                if family == "MAC":
                    full = orc.mac(msg[:off], key)
                    want[k] = full[:6] if k == last_g else full
                elif family == "HASH":
                    full = orc.belt_hash(msg[:off])
                    want[k] = full[:20] if k == last_g else full
                else:
                    code, want[k] = orc.bashHash(SP.BASH_LEVEL[family], msg[:off])
                    assert code == 0
        return want
    if family[:3] in ("ECB", "CBC") and len(msg) % 16:
        # stealing (belt_ecb.c:74-83, belt_cbc.c:86-93,118-130) rewrites the last whole block and the tail, both inside the last step
        assert ops[-1][1] > 16
    off = 0
    for k, (_, n) in enumerate(ops):
        want[k] = whole[off:off + n]
        off += n
    return want


def _ctr_states(orc, key, iv, pieces_e):
    """the oracle's own belt_ctr_st after every E / D step (None for the others)"""
    ost = ctypes.create_string_buffer(72)
    orc.lib.orc_beltCTRStart(ost, key, _sz(len(key)), iv)
    out = []
    for p in pieces_e:
        if p is None:
            out.append(None)
            continue
        buf = ctypes.create_string_buffer(p, len(p))
        orc.lib.orc_beltCTRStepE(buf, _sz(len(p)), ost)
        out.append(ost.raw)
    return out


def _masked(family, state):
    if family == "MAC":
        filled, = struct.unpack_from("<Q", state, 96)              # belt_mac_st: key 32, s 16, r 16, mac 16, block 16, filled
        assert filled <= 16
        return state[:80 + filled] + bytes(16 - filled) + state[96:]
    return state


def _check_outputs(family, name, ops, run, want, tag):
    for k, (op, n) in enumerate(ops):
        if op == "V":
            assert run.outs[k] is True, (family, name, tag, k, "the oracle's tag is refused")
        elif want[k] is not None:
            assert run.outs[k] == want[k], (family, name, tag, k, op, n)


# --------------------------------------------------------------- a / b: forced ---
_cache = {}


def _forced_runs(orc, family, klen):
    """every plan of the family under the three alternating patterns and under all-GPU / all-host, once per (family, key length)"""
    if (family, klen) in _cache:
        return _cache[family, klen]
    L = _lib()
    key, iv = _key(orc, klen), _iv(orc)
    out = {}
    for pi, (name, ops) in enumerate(SP.plans(family).items()):
        pieces = _pieces(orc, ops, 0x5A0 + 16 * klen + pi)
        want = expected(orc, family, ops, pieces, key, iv)
        pats = {p: SP.pattern(p, len(ops) + 1, seed=klen + pi) for p in SP.PATTERNS}
        pats["all-g"], pats["all-c"] = "g" * (len(ops) + 1), "c" * (len(ops) + 1)
        out[name] = (ops, pieces, want, pats, {p: run_plan(L, family, ops, pieces, key, iv, pat, want) for p, pat in pats.items()})
    _cache[family, klen] = out
    return out


UNKEYED = ("HASH",) + tuple(SP.BASH_LEVEL)
CASES = [(f, k) for f in SP.FAMILIES for k in ((32,) if f in UNKEYED else KEY_LENS)]      # key lengths 16, 24, 32 where there is a key


@pytest.mark.parametrize("family,klen", CASES)
def test_forced_alternation_matches_the_oracle(orc, family, klen):
    for name, (ops, pieces, want, pats, runs) in _forced_runs(orc, family, klen).items():
        steps = SP.simulate(family, ops)
        for p in SP.PATTERNS:
            run, pat = runs[p], pats[p]
            _check_outputs(family, name, ops, run, want, p)
            for k, (d0, d1, d2) in enumerate(run.deltas):
                where = (family, name, p, k, ops[k], pat[k + 1])
                assert d2 == 0, where
                assert (d0 if pat[k + 1] == "g" else d1) == 0, where
                assert d0 + d1 == len(steps[k].calls), where                # the model of streamplans counts the helper calls
    # a damaged tag is refused by either engine, whichever engine absorbed the data
    if family in ("DWP", "CHE", "MAC"):
        L = _lib()
        key, iv = _key(orc, klen), _iv(orc)
        name = "unwrap" if family != "MAC" else "aligned"
        ops, pieces, want, pats, _ = _forced_runs(orc, family, klen)[name]
        bad = [None if w is None else bytes([w[0] ^ 1]) + w[1:] for w in want]
        vs = [k for k, (op, _) in enumerate(ops) if op == "V"]
        for p in ("gc", "cg"):
            run = run_plan(L, family, ops, pieces, key, iv, pats[p], bad)
            assert vs and [run.outs[k] for k in vs] == [False] * len(vs), (family, p)


@pytest.mark.parametrize("family,klen", CASES)
def test_state_after_each_step_is_the_same_from_either_engine(orc, family, klen):
    key, iv = _key(orc, klen), _iv(orc)
    for name, (ops, pieces, want, pats, runs) in _forced_runs(orc, family, klen).items():
        ref_g, ref_c = runs["all-g"], runs["all-c"]
        _check_outputs(family, name, ops, ref_g, want, "all-g")
        _check_outputs(family, name, ops, ref_c, want, "all-c")
        for p in SP.PATTERNS + ("all-c",):
            for k in range(len(ops)):
                a, g, c = (_masked(family, r.states[k]) for r in (runs[p], ref_g, ref_c))
                assert a == g, (family, name, p, k, ops[k], "differs from the all-GPU run", _diff(a, g))
                assert a == c, (family, name, p, k, ops[k], "differs from the all-host run", _diff(a, c))
        # ... and against the oracle where it has the same state
        if family in ("CTR", "DWP"):
            ost = _ctr_states(orc, key, iv, [p if op in "ED" else None for (op, _), p in zip(ops, pieces)])
            for p in SP.PATTERNS + ("all-g", "all-c"):
                for k in range(len(ops)):
                    if ost[k] is not None:
                        assert runs[p].states[k][:72] == ost[k], (family, name, p, k, ops[k])
        if family[:3] == "BDE" or family == "CHE":
            s, done = orc.block_encr(iv, key), 0                  # s0 = E_K(iv) (belt_bde.c:47, belt_che.c:54-57)
            at = 32 if family != "CHE" else 144                   # belt_bde_st.s; belt_che_st.s behind the belt_dwp_st
            for k, (op, n) in enumerate(ops):
                if op in "ED":
                    blocks = (done + n + 15) // 16 - (done + 15) // 16        # a partial block has taken its s already
                    done += n
                    if family == "CHE":
                        _, s = orc.che_blocks_from(bytes(16 * blocks), key, s)
                    else:
                        _, s = orc.bde_blocks_from(bytes(16 * blocks), key, s, decr=family[-1] == "D")
                for p in SP.PATTERNS + ("all-g", "all-c"):
                    assert runs[p].states[k][at:at + 16] == s, (family, name, p, k, ops[k])


def _diff(a, b):
    return [i for i in range(len(a)) if a[i] != b[i]][:24]


# ------------------------------------------------------------------ c: auto mode ---
_clmul = {}


def _host_has_clmul(L, orc):
    """which polynomial crossover this host has (32 KiB with PCLMULQDQ, 4 KiB without): ONE probe step of 8192 octets may go either
    way; everything else must then be consistent with it"""
    if id(L) not in _clmul:
        L.bee2hip_path_policy(0)
        key, iv = _key(orc, 32), _iv(orc)
        st = _start(L, "DWP", key, iv)
        c0 = _counts(L)
        L.beltDWPStepI(orc.fill(8192, 0xC1), _sz(8192), st)
        d = tuple(b - a for a, b in zip(c0, _counts(L)))
        assert d in ((1, 0, 0), (0, 1, 0)), d
        _clmul[id(L)] = d == (1, 0, 0)
    return _clmul[id(L)]


@pytest.mark.parametrize("family", SP.CROSSOVER_FAMILIES)
def test_auto_mode_takes_the_engine_the_thresholds_predict(orc, family):
    L = _lib()
    clmul = _host_has_clmul(L, orc)
    klen = KEY_LENS[SP.CROSSOVER_FAMILIES.index(family) % 3]
    key, iv = _key(orc, klen), _iv(orc)
    seen = set()
    for pi, (name, ops) in enumerate(SP.plans(family).items()):
        pieces = _pieces(orc, ops, 0xA070 + pi)
        want = expected(orc, family, ops, pieces, key, iv)
        run = run_plan(L, family, ops, pieces, key, iv, "a" * (len(ops) + 1), want)
        _check_outputs(family, name, ops, run, want, "auto")
        for k, st in enumerate(SP.simulate(family, ops)):
            host, gpu = SP.predicted_counts(st, clmul)
            assert run.deltas[k] == (host, gpu, 0), (family, name, k, ops[k], st.calls, "PCLMULQDQ" if clmul else "table")
            seen |= {(kind, SP.host_in_auto(kind, b, clmul)) for kind, b in st.calls}
    for op in {o for ops in SP.plans(family).values() for o, _ in ops if o not in "GV"}:
        kind = SP.bulk_kind(family, op)
        assert (kind, True) in seen and (kind, False) in seen, (family, kind)       # both engines did serve the stream


_TEXT = (0, 7, 8191, 8192, 40001)
_HEADER = (0, 5, 4096, 40000)


@pytest.mark.parametrize("mode", ["DWP", "CHE"])
def test_auto_mode_wrap_and_unwrap_with_parts_on_different_sides(orc, mode):
    L = _lib()
    clmul = _host_has_clmul(L, orc)
    iv = _iv(orc)
    start_prims = 2 if mode == "DWP" else 1            # E_K(iv) and, for belt-dwp, r = E_K of it (capi_belt.hip:349-351,648)
    wrap, unwrap = getattr(L, f"belt{mode}Wrap"), getattr(L, f"belt{mode}Unwrap")
    for ci, (hl, tl) in enumerate((h, t) for h in _HEADER for t in _TEXT):
        key = _key(orc, KEY_LENS[ci % 3])
        hdr, text = orc.fill(hl, 0x4EAD + ci), orc.fill(tl, 0x7E87 + ci)
        code, ct_want, mac_want = orc.dwp_wrap(text, hdr, key, iv, mode=mode)
        assert code == 0
        where = (mode, hl, tl, "PCLMULQDQ" if clmul else "table")
        # wrap: I, E, A, G
        steps = SP.simulate(mode, [("I", hl), ("E", tl), ("A", tl), ("G", 0)])
        host = sum(SP.predicted_counts(s, clmul)[0] for s in steps) + start_prims
        gpu = sum(SP.predicted_counts(s, clmul)[1] for s in steps)
        dest, mac = ctypes.create_string_buffer(max(tl, 1)), ctypes.create_string_buffer(8)
        c0 = _counts(L)
        assert wrap(dest, mac, text, _sz(tl), hdr, _sz(hl), key, _sz(len(key)), iv) == 0, where
        assert tuple(b - a for a, b in zip(c0, _counts(L))) == (host, gpu, 0), where
        assert dest.raw[:tl] == ct_want and mac.raw == mac_want, where
        # unwrap: I, A, V, D
        steps = SP.simulate(mode, [("I", hl), ("A", tl), ("V", 0), ("D", tl)])
        host = sum(SP.predicted_counts(s, clmul)[0] for s in steps) + start_prims
        gpu = sum(SP.predicted_counts(s, clmul)[1] for s in steps)
        dest = ctypes.create_string_buffer(max(tl, 1))
        c0 = _counts(L)
        assert unwrap(dest, ct_want, _sz(tl), hdr, _sz(hl), mac_want, key, _sz(len(key)), iv) == 0, where
        assert tuple(b - a for a, b in zip(c0, _counts(L))) == (host, gpu, 0), where
        assert dest.raw[:tl] == text, where
        # a damaged tag: ERR_BAD_MAC, nothing decrypted, dest untouched
        bad = mac_want[:7] + bytes([mac_want[7] ^ 0x80])
        dest = ctypes.create_string_buffer(b"\xA5" * max(tl, 1), max(tl, 1))
        assert unwrap(dest, ct_want, _sz(tl), hdr, _sz(hl), bad, key, _sz(len(key)), iv) == ERR_BAD_MAC, where
        assert dest.raw == b"\xA5" * max(tl, 1), where
        assert orc.dwp_unwrap(ct_want, hdr, bad, key, iv, mode=mode)[0] == ERR_BAD_MAC


@pytest.mark.parametrize("fn,family,start_prims,lengths", [
    ("beltCTR", "CTR", 1, (7, 8191, 8192, 40001)),
    ("beltECBEncr", "ECB-E", 0, (23, 8191, 8199, 40001)),
    ("beltECBDecr", "ECB-D", 0, (23, 8191, 8199, 40001)),
    ("beltCBCDecr", "CBC-D", 0, (8191, 8192, 8215, 40001)),
    ("beltBDEEncr", "BDE-E", 1, (16, 8176, 8192, 40000)),
    ("beltBDEDecr", "BDE-D", 1, (16, 8176, 8192, 40000)),
])
def test_auto_mode_one_shot_calls_on_both_sides_of_the_crossover(orc, fn, family, start_prims, lengths):
    L = _lib()
    clmul = _host_has_clmul(L, orc)
    iv = _iv(orc)
    engines = set()
    for ci, n in enumerate(lengths):
        key = _key(orc, KEY_LENS[ci % 3])
        src = orc.fill(n, 0x0E5 + n)
        want = expected(orc, family, [(family[-1] if family != "CTR" else "E", n)], [src], key, iv)[0]
        step, = SP.simulate(family, [("E" if family == "CTR" else family[-1], n)])
        host, gpu = SP.predicted_counts(step, clmul)
        engines |= {gpu > 0}
        dest = ctypes.create_string_buffer(n)
        args = (dest, src, _sz(n), key, _sz(len(key))) + (() if family[:3] == "ECB" else (iv,))
        c0 = _counts(L)
        assert getattr(L, fn)(*args) == 0, (fn, n)
        assert tuple(b - a for a, b in zip(c0, _counts(L))) == (host + start_prims, gpu, 0), (fn, n)
        assert dest.raw == want, (fn, n)
    assert engines == {True, False}


# ------------------------------------------------- d: software fallback in mid-stream ---
@pytest.mark.parametrize("family,ops,hit", [
    # whole blocks: no partial block exists in a belt-bde state
    ("BDE-E", [("E", 48), ("E", 20000), ("E", 16), ("E", 8192), ("E", 32)], 1),
    # 5 leaves 11 octets of gamma; 8206 = the 11, 8192 through the failing device call, 3 into a new gamma block
    ("CHE", [("I", 21), ("E", 5), ("E", 8206), ("A", 8211), ("E", 20000), ("E", 9), ("A", 20009), ("G", 0), ("V", 0)], 2),
    # 5 buffered; 40014 = 11 to fill the block (host), 40000 through the failing device call, 3 buffered again
    ("DWP", [("I", 7), ("A", 5), ("A", 40014), ("A", 9), ("E", 8197), ("A", 40000), ("E", 30), ("G", 0), ("V", 0)], 2),
])
def test_device_failure_in_mid_stream_is_finished_on_the_host(orc, family, ops, hit):
    """tune 5 = 2: the next two device attempts of a drop-in helper report a failure without running (staging.hpp with_host), so the
    step's bulk call is finished by the host path -- from the state the earlier steps left, into the state the later steps use"""
    L = _lib(exp=True)
    clmul = _host_has_clmul(L, orc)
    key, iv = _key(orc, 24), _iv(orc)
    pieces = _pieces(orc, ops, 0xFA11)
    want = expected(orc, family, ops, pieces, key, iv)
    steps = SP.simulate(family, ops)
    assert steps[hit].pending_before != 0 or family in SP.NO_PENDING_FIELD
    assert SP.predicted_counts(steps[hit], clmul)[1] == 1                  # exactly one call of the step goes to the device
    auto = "a" * (len(ops) + 1)
    clean = run_plan(L, family, ops, pieces, key, iv, auto, want)
    _check_outputs(family, "fallback", ops, clean, want, "clean")

    def arm(k):
        L.bee2hip_internal_tune(5, 2 if k == hit else 0)
    try:
        run = run_plan(L, family, ops, pieces, key, iv, auto, want, before_step=arm)
    finally:
        L.bee2hip_internal_tune(5, 0)
    _check_outputs(family, "fallback", ops, run, want, "injected")         # the step itself and the rest of the stream
    for k, st in enumerate(steps):
        host, gpu = SP.predicted_counts(st, clmul)
        assert run.deltas[k] == ((host, 0, 1) if k == hit else (host, gpu, 0)), (family, k, ops[k])
        assert clean.deltas[k] == (host, gpu, 0), (family, k, ops[k])
        assert run.states[k] == clean.states[k], (family, k, ops[k], _diff(run.states[k], clean.states[k]))
    # the state after the step against the oracle, where it has one: the counter block of belt-dwp, the tweak of belt-bde / belt-che
    if family == "DWP":
        ost = _ctr_states(orc, key, iv, [p if op in "ED" else None for (op, _), p in zip(ops, pieces)])
        assert all(run.states[k][:72] == ost[k] for k in range(len(ops)) if ost[k] is not None)
    else:
        s, done, at = orc.block_encr(iv, key), 0, 144 if family == "CHE" else 32
        for k, (op, n) in enumerate(ops):
            if op in "ED":
                blocks = (done + n + 15) // 16 - (done + 15) // 16
                done += n
                _, s = orc.che_blocks_from(bytes(16 * blocks), key, s) if family == "CHE" else orc.bde_blocks_from(bytes(16 * blocks), key, s)
            assert run.states[k][at:at + 16] == s, (family, k, ops[k])
