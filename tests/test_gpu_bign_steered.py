"""-m gpu: the steered signatures of tests/golden/bign_steered.json (tests/steered.py) through every form that walks R = u G + v Q on
the three standard curves -- the general batch entry with each kernel set forced, the one-signer and the keyed entries on both table
forms with one and four lanes per signature, the drop-in calls on the host and on the GPU.  Every verdict is the fixture's, which is
the reference's.  Only a VALID signature can show a wrong walk (a damaged one is ERR_BAD_SIG whatever the arithmetic did), so what is
fed here are valid signatures whose u has zero comb windows, is 0, 1 or q - 1, whose s0 has empty windows under a shared key, whose
accumulator meets +-(the comb point it is about to add) at a chosen step -- and, for a kernel that skips a window it should have
added, their invalid neighbours."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import steered as ST
from bee2_amd import engine as E
from gpulib import dev, exp_engine

pytestmark = pytest.mark.gpu
ORDINARY = 257
PATHS = [(128, p) for p in (1, 2, 3, 0x43, 0x23, 0x83, 0)] + [(l, p) for l in (192, 256) for p in (1, 3, 0)]     # 0: unforced
TABLE_FORMS = [(63, 1), (63, 0), (0, 1), (0, 0)]       # (tune 20, tune 22): the 8-bit table first -- a key keeps a 16-bit table it has


def _ordinary(golden, l, n):
    """n valid (hash, sig, pubkey) of the reference's base fixtures"""
    if l == 128:
        base = golden.bign_base
    else:
        base = [tuple(bytes.fromhex(t[k]) for k in ("hash", "sig", "pubkey")) for t in golden.bign_big[str(l)]["base"]]
    return [base[i % len(base)] for i in range(n)]


@functools.lru_cache(maxsize=None)
def _general_batches(l):
    """-> [(name, hashes, sigs, pubkeys, codes)]: uniform = every case 64 times back to back (a whole wavefront takes the rare
    branch together), mixed = the cases among 257 ordinary signatures, shuffled (the branch diverges)"""
    import orclib
    fx = ST.load()
    cases = [(c["hash"], c["sig"], c["pubkey"], c["code"]) for c in fx.of(l)]
    uniform = [x for x in cases for _ in range(64)]
    mixed = cases + [t + (0,) for t in _ordinary(orclib.Golden(), l, ORDINARY)]
    mixed = [mixed[i] for i in np.random.default_rng(0x57EE + l).permutation(len(mixed))]
    return [(name, b"".join(x[0] for x in b), b"".join(x[1] for x in b), b"".join(x[2] for x in b), np.array([x[3] for x in b], dtype=np.int64))
            for name, b in (("uniform", uniform), ("mixed", mixed))]


def _got(codes):
    torch.cuda.synchronize()
    return codes.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def _tuner(eng):
    tune, stat = eng.lib.bee2hip_internal_tune, eng.lib.bee2hip_internal_stat
    tune.restype = ctypes.c_uint32
    stat.restype = ctypes.c_ulonglong
    return tune, stat


@pytest.mark.parametrize("l,path", PATHS)
def test_general_entry_every_kernel_set(l, path):
    """bignVerifyL_batch_dev with each kernel set FORCED (bee2hip_internal_tune 2: 32-bit limbs, 29-bit limbs, quads / pairs by size,
    quads, pairs, quad + helper quad -- the form whose last addition v Q + u G the "fold E" case makes a doubling) and unforced"""
    eng = exp_engine()
    tune, _ = _tuner(eng)
    assert tune(2, path) == 0
    try:
        for name, H, S, K, want in _general_batches(l):
            codes = torch.full((want.size,), -1, dtype=torch.int32, device="cuda")
            eng.bignVerifyL_batch_dev(l, E.LEVEL_OID[l], dev(H), dev(S), dev(K), codes)
            got = _got(codes)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (name, bad[:8], got[bad[:8]], want[bad[:8]])
            assert int((want == 0).sum()) > want.size // 2 and int((want == ST.ERR_BAD_SIG).sum()) > want.size // 8
    finally:
        tune(2, 0)


def _interleave(groups):
    """round robin over the groups until all are used up"""
    out, its = [], [iter(g) for g in groups]
    while its:
        for it in list(its):
            x = next(it, None)
            if x is None:
                its.remove(it)
            else:
                out.append(x)
    return out


def _key_batches(orc, l):
    """-> [(pubkey, items)] per distinct key, items = [(hash, sig, code)]: 70 copies of every case under the key and 10 ordinary
    signatures under it (the fixture's pool; made by the oracle's signer where the fixture keeps d), interleaved"""
    fx = ST.load()
    by_key = {}
    for c in fx.of(l):
        by_key.setdefault(c["pubkey"], []).append(c)
    signer = {s["pubkey"]: s for s in fx.signers[l]}
    out = []
    for pub, cs in by_key.items():
        copies = 70 if cs[0]["family"] != "c" else 10
        groups = [[(c["hash"], c["sig"], c["code"])] * copies for c in cs]
        s = signer.get(pub)
        if s is not None:
            pool = list(s["pool"])
            if s["d"] is not None:
                priv = s["d"].to_bytes(l // 4, "little")
                for i in range(10):
                    h = orc.fill(l // 4, 0x900D + 16 * l + i)
                    code, sig = orc.sign2(l, E.LEVEL_OID[l], h, priv)
                    assert code == 0
                    pool.append((h, sig))
            assert len(pool) >= 10
            groups.append([(h, g, 0) for h, g in pool])
        out.append((pub, _interleave(groups)))
    return out


@pytest.mark.parametrize("l", ST.LEVELS)
def test_one_signer_entry_per_key(orc, l):
    """bignVerifyL_onekey_batch_dev, one call per distinct key of the fixture, on the key's 8-bit and its 16-bit table (tune 20) with
    four lanes and one lane per signature (tune 22); family c as one batch of its signer's seven cases and its pool.  The cache starts
    empty for every key (tune 23), so the 16-bit table is known to be there when it is asked for (stat 5)"""
    eng = exp_engine()
    tune, stat = _tuner(eng)
    batches = _key_batches(orc, l)
    assert len(batches) >= 2 * ST.nw(l) + 17 + 1 + 7
    try:
        for pub, items in batches:
            assert tune(23, 0) == 0 and stat(5) == 0
            H, S = dev(b"".join(x[0] for x in items)), dev(b"".join(x[1] for x in items))
            want = np.array([x[2] for x in items], dtype=np.int64)
            for t16, quads in TABLE_FORMS:
                assert tune(20, t16) == 0 and tune(22, quads) == 0
                codes = torch.full((want.size,), -1, dtype=torch.int32, device="cuda")
                eng.bignVerifyL_onekey_batch_dev(l, E.LEVEL_OID[l], H, S, pub, codes)
                got = _got(codes)
                assert stat(5) == (1 if t16 == 0 else 0)
                bad = np.nonzero(got != want)[0]
                assert bad.size == 0, (pub.hex()[:16], t16, quads, bad[:8], got[bad[:8]], want[bad[:8]])
    finally:
        tune(20, -1); tune(22, -1); tune(23, 0)


@pytest.mark.parametrize("l", ST.LEVELS)
def test_keyed_entry_all_cases_in_one_call(l):
    """bignVerifyL_keyed_batch_dev: every case of the curve and the pool of family c's signer in ONE call, the keys deduplicated (the
    seven cases of family c and the neighbours of family e share theirs), under the same four settings"""
    eng = exp_engine()
    tune, stat = _tuner(eng)
    fx = ST.load()
    items = [(c["hash"], c["sig"], c["pubkey"], c["code"]) for c in fx.of(l)]
    items += [(h, g, s["pubkey"], 0) for s in fx.signers[l] for h, g in s["pool"]]
    items = [items[i] for i in np.random.default_rng(0xE1ED + l).permutation(len(items))]
    keys = sorted({x[2] for x in items})
    pos = {k: i for i, k in enumerate(keys)}
    assert len(keys) < len(fx.of(l)) - 7 and len(keys) <= 96
    H, S = dev(b"".join(x[0] for x in items)), dev(b"".join(x[1] for x in items))
    idx = torch.from_numpy(np.array([pos[x[2]] for x in items], dtype=np.int32)).cuda()
    want = np.array([x[3] for x in items], dtype=np.int64)
    try:
        assert tune(23, 0) == 0 and stat(5) == 0
        for t16, quads in TABLE_FORMS:
            assert tune(20, t16) == 0 and tune(22, quads) == 0
            codes = torch.full((want.size,), -1, dtype=torch.int32, device="cuda")
            eng.bignVerifyL_keyed_batch_dev(l, E.LEVEL_OID[l], H, S, b"".join(keys), idx, codes)
            got = _got(codes)
            assert stat(5) == (len(keys) if t16 == 0 else 0)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, (t16, quads, bad[:8], got[bad[:8]], want[bad[:8]])
    finally:
        tune(20, -1); tune(22, -1); tune(23, 0)


@pytest.mark.parametrize("force", [0, 1])
@pytest.mark.parametrize("l", ST.LEVELS)
def test_drop_in_calls(l, force):
    """bignVerify and bign128Verify / bign192Verify / bign256Verify on every case: in auto mode (one signature: the host path,
    host_bign.hpp) and with every call forced into the kernels (tune 4 = 1, as BEE2HIP_FORCE=gpu)"""
    eng = exp_engine()
    tune, stat = _tuner(eng)
    params = eng.bignParamsStd(E.CURVE_NAME[l])
    host0, fell0 = stat(0), stat(2)
    assert tune(4, force) == 0
    try:
        bad = []
        for c in ST.load().of(l):
            a = eng.bignVerify(params, E.LEVEL_OID[l], c["hash"], c["sig"], c["pubkey"]) & 0xFFFFFFFF
            b = eng.bignLVerify(l, c["hash"], c["sig"], c["pubkey"]) & 0xFFFFFFFF
            if (a, b) != (c["code"], c["code"]):
                bad.append((c["family"], c["name"], a, b, c["code"]))
        assert not bad, bad[:8]
        assert stat(0) - host0 == (0 if force else 2 * len(ST.load().of(l))) and stat(2) == fell0      # host-path calls; none finished there after a fault
    finally:
        tune(4, 0)
