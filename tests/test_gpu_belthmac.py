"""-m gpu: the belt-hmac / belt-pbkdf2 batches (bee2hip_beltHMAC_*ragged*, bee2hip_beltPBKDF2_batch*,
bee2_amd/csrc/belt_hmac_kernels.hip) and the two one-shots against the model, record by record, every output octet compared
(tests/belthmacgrid.py builds the batches; tests/test_belthmac.py pins the model to the reference and the kernel's per-lane
logic to the model on the CPU).

The stream entries are device-pointer batch entries that are not in the contract registry of tests/devcontract.py, so this
file holds them to the same contract itself, as tests/test_gpu_beltkwp.py does: every buffer is a slice of one allocation
filled with a seeded pattern, at the weakest alignment the header grants, with 4 KiB of pattern on each side; after a call the
outputs are the model's over their whole range and every other octet of the allocation -- inputs and guards -- is what it
was."""
import functools
import json
import os
import random
import struct

import numpy as np
import pytest
import torch

import belthmacgrid as G
import orc_belthmac as M
import orclib
from bee2_amd import engine as E
from gpulib import engine

pytestmark = pytest.mark.gpu
GUARD = 4096
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def pack64(v):
    return struct.pack(f"<{len(v)}Q", *v)


def hmac_arena(b, mac_len, macs=None, data_off=1, key_off=3, mac_off=5, order=None, seed=1, first=0):
    """data, keys and MACs at odd addresses unless told otherwise; the offsets 8-aligned, order and codes 4 mod 8.  macs given:
    the arena of a verifying call.  first: the offsets start there (octets of pattern in front of the first record)"""
    A = Arena(seed).add("data", bytes(first) + b"".join(b.msgs), data_off).add("offs", pack64(G.offsets(b.msg_lens, first)))
    if b.key is None:
        A.add("keys", b"".join(b.keys), key_off).add("koffs", pack64(G.offsets(b.key_lens)))
    if order is not None:
        A.add("order", struct.pack(f"<{b.n}I", *order), 4)
    if macs is None:
        A.add("macs", b.n * mac_len, mac_off)
    else:
        A.add("macs", b"".join(macs), mac_off).add("codes", 4 * b.n, 4)
    return A.build()


def hmac_call(eng, b, A, mac_len):
    verify = "codes" in A.at
    eng.beltHMAC_ragged_stream(1 if verify else 0, b.key, A.t("keys") if b.key is None else None,
                               A.t("koffs") if b.key is None else None, A.t("data"), A.t("offs"),
                               A.t("order") if "order" in A.at else None, b.n, A.t("macs"), mac_len,
                               A.t("codes") if verify else None)


def run_macs(eng, b, mac_len=32, **kw):
    A = hmac_arena(b, mac_len, **kw)
    hmac_call(eng, b, A, mac_len)
    got = A.fetch(["macs"])["macs"]
    return [got[mac_len * i:mac_len * (i + 1)] for i in range(b.n)]


def run_verify(eng, b, macs, **kw):
    mac_len = len(macs[0])
    A = hmac_arena(b, mac_len, macs=macs, **kw)
    hmac_call(eng, b, A, mac_len)
    return list(struct.unpack(f"<{b.n}I", A.fetch(["codes"])["codes"]))


def spoil(macs, every=5, start=2):
    """a bit of the LAST octet flipped in every 5th MAC -> (macs, [codes])"""
    out, codes = [], []
    for i, m in enumerate(macs):
        bad = i % every == start
        out.append(m[:-1] + bytes([m[-1] ^ (0x80 >> (i % 8))]) if bad else m)
        codes.append(E.ERR_BAD_MAC if bad else 0)
    return out, codes


def check(eng, b, mac_len=32, **kw):
    """writing, verifying the result, and verifying it with every 5th MAC spoilt in its last compared octet"""
    want = [m[:mac_len] for m in b.want()]
    got = run_macs(eng, b, mac_len, **kw)
    bad = [i for i in range(b.n) if got[i] != want[i]]
    assert not bad, (b.n, mac_len, [(i, b.key_lens[i], b.msg_lens[i]) for i in bad[:8]])
    assert run_verify(eng, b, want, **kw) == [0] * b.n
    macs, codes = spoil(want)
    assert run_verify(eng, b, macs, **kw) == codes


# ================================================================================================ shapes
def test_per_record_keys_over_every_key_and_message_length():
    """every fixture key length x message length in one batch of 143, shuffled: each wavefront holds zero-padded and hashed
    keys, the empty message and every tail residue at once"""
    b = G.grid_batch()
    assert {(k, m) for k, m in zip(b.key_lens, b.msg_lens)} == {(k, m) for k in G.KEY_LENS for m in G.MSG_LENS}
    check(engine(), b)


@pytest.mark.parametrize("n", G.BATCH_SIZES)
def test_per_record_keys_at_every_batch_edge(n):
    """one record, a partial, a whole and a started second wavefront, five wavefronts with the order built on the device"""
    check(engine(), G.batch(n))


@pytest.mark.parametrize("key_len", [0, 29, 32, 33, 97])
def test_shared_key_over_the_same_messages(key_len):
    """the key's state computed once on the host: an empty key, a padded one, 32 octets as they are, hashed ones"""
    eng = engine()
    check(eng, G.grid_batch(shared=key_len))
    check(eng, G.batch(257, shared=key_len))


def test_fixture_rows_come_out_of_a_batch():
    """the reference's own outputs (tests/golden/belt_hmac.json), all HMAC rows as one batch"""
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "belt_hmac.json")))
    rows = [r for r in fx["rows"] if r["kind"] == "hmac"]
    pairs = [G.case_inputs(r) for r in rows]
    code, macs = engine().beltHMAC_ragged([p[0] for p in pairs], [p[1] for p in pairs])
    assert code == 0 and [m.hex() for m in macs] == [r["out"] for r in rows]


@pytest.mark.parametrize("mac_len", [1, 8, 17, 32])
def test_mac_len_is_what_is_written_and_what_is_compared(mac_len):
    """mac_len octets a record and nothing behind mac_len * n (the arena's guard); a flipped bit in the last compared octet
    refuses that record only; bits flipped just past mac_len -- in the octets of the full MAC that are not handed over, and in
    the octet behind the last record -- change nothing"""
    eng = engine()
    b = G.batch(65, seed=mac_len)
    check(eng, b, mac_len)
    b = G.batch(65, shared=31, seed=mac_len)
    check(eng, b, mac_len, mac_off=0)
    want = [m[:mac_len] for m in b.want()]
    A = hmac_arena(b, mac_len, macs=want, seed=9)
    s, n = A.at["macs"]
    A.image[s + n] ^= 0x01                                          # the octet behind the last MAC
    A.refill()
    hmac_call(eng, b, A, mac_len)
    assert A.fetch(["codes"])["codes"] == bytes(4 * b.n)


# ================================================================================================ alignments
def test_every_start_alignment_of_the_data():
    """the data base at 0..15 mod 16 (the reader's quad, dword and octet shifts), the first record's offset moving with it, so
    that records start at every residue; keys and MACs elsewhere"""
    eng = engine()
    b = G.batch(65, seed=3)
    for a in range(16):
        check(eng, b, data_off=a, key_off=(a + 1) % 4, mac_off=(a + 2) % 4, first=(5 * a) % 16)


def test_every_start_alignment_of_keys_and_macs():
    eng = engine()
    b = G.batch(65, seed=4)
    for a in range(4):
        for mac_len in (32, 20, 7):
            check(eng, b, mac_len, data_off=0, key_off=a, mac_off=(a + 1) % 4)
            check(eng, b, mac_len, data_off=2, key_off=(a + 2) % 4, mac_off=a)


def test_a_record_may_end_where_its_allocation_ends():
    """data, keys and salts that end with the allocation's last octet: a quad without an octet of the record is never
    loaded, so nothing is read behind it"""
    eng = engine()
    b = G.batch(65, seed=6)
    data, keys = b"".join(b.msgs), b"".join(b.keys)
    dt = torch.empty(len(data), dtype=torch.uint8, device="cuda")
    kt = torch.empty(len(keys), dtype=torch.uint8, device="cuda")
    dt.copy_(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()))
    kt.copy_(torch.from_numpy(np.frombuffer(keys, dtype=np.uint8).copy()))
    offs = torch.tensor(G.offsets(b.msg_lens), dtype=torch.int64, device="cuda")
    koffs = torch.tensor(G.offsets(b.key_lens), dtype=torch.int64, device="cuda")
    macs = torch.zeros(32 * b.n, dtype=torch.uint8, device="cuda")
    eng.beltHMAC_ragged_stream(0, None, kt, koffs, dt, offs, None, b.n, macs, 32)
    torch.cuda.synchronize()
    assert macs.cpu().numpy().tobytes() == b"".join(b.want())


# ================================================================================================ one long record
@functools.lru_cache(maxsize=None)
def long_batch():
    b = G.Batch(257, seed=11)
    b.msg_lens[100] = 4096 + 5
    b.msgs[100] = random.Random(12).randbytes(4096 + 5)
    return b


@pytest.mark.parametrize("order", ["none", "identity", "reverse"])
def test_one_long_record_among_256_short_ones(order):
    """4096 + 5 octets in ONE lane (no multi-lane form here) while its wavefront's other lanes are done early; with the
    order built on the device, given as the identity, and reversed"""
    b = long_batch()
    ords = {"none": None, "identity": list(range(257)), "reverse": list(range(256, -1, -1))}
    check(engine(), b, order=ords[order])


# ================================================================================================ PBKDF2
@functools.lru_cache(maxsize=None)
def kdf(pwd, it, salt):
    return M.pbkdf2(pwd, it, salt)


def kdf_arena(pwds, salts, salt_len, stride, n, key_off=1, pwd_off=3, salt_off=5, order=None, seed=2):
    A = Arena(seed).add("pwds", b"".join(pwds), pwd_off).add("poffs", pack64(G.offsets([len(p) for p in pwds])))
    A.add("salts", salts, salt_off).add("keys", 32 * n, key_off)
    if order is not None:
        A.add("order", struct.pack(f"<{n}I", *order), 4)
    return A.build()


def kdf_call(eng, A, it, salt_len, stride, n):
    eng.beltPBKDF2_batch_stream(A.t("pwds"), A.t("poffs"), it, A.t("salts"), salt_len, stride,
                                A.t("order") if "order" in A.at else None, n, A.t("keys"))


def kdf_case(n, salt_len, stride_kind, seed, rot=None):
    """passwords of the fixture's key lengths, the list walked from position rot (seed when not given); stride_kind 0: one
    salt, 1: salt_len apart, 2: salt_len + 3 apart"""
    rnd = random.Random(1000 * salt_len + 10 * n + stride_kind + 7 * seed)
    rot = seed if rot is None else rot
    pwds = [rnd.randbytes(G.KEY_LENS[(i + rot) % len(G.KEY_LENS)]) for i in range(n)]
    stride = (0, salt_len, salt_len + 3)[stride_kind]
    raw = rnd.randbytes((n - 1) * stride + salt_len)
    return pwds, raw, stride, [raw[i * stride:i * stride + salt_len] for i in range(n)]


@pytest.mark.parametrize("it", G.ITERS)
def test_pbkdf2_over_salt_lengths_and_strides(it):
    """salt lengths with the suffix 00 00 00 01 inside a block, filling it, straddling two and starting one; one salt for the
    batch, salts back to back, salts 3 octets apart; passwords short and hashed; a second wavefront started"""
    eng = engine()
    for salt_len in G.SALT_LENS:
        for kind in range(3):
            if salt_len == 0 and kind == 1:
                continue                                              # (stride 0 again)
            n = 65 if it < 50 else 21
            pwds, raw, stride, salts = kdf_case(n, salt_len, kind, it)
            A = kdf_arena(pwds, raw, salt_len, stride, n, key_off=(salt_len + kind) % 4, salt_off=(salt_len + 2 * kind) % 16)
            kdf_call(eng, A, it, salt_len, stride, n)
            got = A.fetch(["keys"])["keys"]
            want = [kdf(pwds[i], it, salts[i]) for i in range(n)]
            bad = [i for i in range(n) if got[32 * i:32 * i + 32] != want[i]]
            assert not bad, (it, salt_len, stride, [(i, len(pwds[i])) for i in bad[:8]])


@pytest.mark.parametrize("n", G.BATCH_SIZES)
def test_pbkdf2_at_every_batch_edge_ordered_by_password_length(n):
    eng = engine()
    pwds, raw, stride, salts = kdf_case(n, 8, 1, 3)
    for order in (None, list(range(n - 1, -1, -1))):
        A = kdf_arena(pwds, raw, 8, stride, n, order=order)
        kdf_call(eng, A, 3, 8, stride, n)
        assert A.fetch(["keys"])["keys"] == b"".join(kdf(pwds[i], 3, salts[i]) for i in range(n))


def test_pbkdf2_fixture_rows_and_the_published_vectors_inside_batches():
    """the reference's rows at each iteration count as one batch per (iter, salt length); the 10 000- and 2048-iteration
    vectors of the reference's tests as record 1 of 3"""
    eng = engine()
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "belt_hmac.json")))
    for it in G.ITERS:
        for mlen in G.MSG_LENS:
            rows = [r for r in fx["rows"] if r["kind"] == "pbkdf2" and r["iter"] == it and r["msg_len"] == mlen]
            pairs = [G.case_inputs(r) for r in rows]
            code, keys = eng.beltPBKDF2_batch([p[0] for p in pairs], it, [p[1] for p in pairs])
            assert code == 0 and [k.hex() for k in keys] == [r["out"] for r in rows], (it, mlen)
    for v in fx["pbkdf2"]:
        pwd, salt = v["pwd"].encode(), bytes.fromhex(v["salt"])
        others = [(b"", bytes(8)), (b"p" * 40, bytes(range(8)))]
        code, keys = eng.beltPBKDF2_batch([others[0][0], pwd, others[1][0]], v["iter"], [others[0][1], salt, others[1][1]])
        assert code == 0 and keys[1].hex() == v["key"]
        assert keys[0] == kdf(others[0][0], v["iter"], others[0][1]) and keys[2] == kdf(others[1][0], v["iter"], others[1][1])
        if v["iter"] == 2048:                                         # one salt for the batch
            assert eng.beltPBKDF2_batch([b"x", pwd, b"y" * 33], v["iter"], salt)[1][1].hex() == v["key"]


# ================================================================================================ the contract
@pytest.mark.parametrize("form", ["write", "verify", "write-shared", "pbkdf2"])
def test_side_stream_and_replay_from_a_graph_on_fresh_inputs(form):
    """one eager call on a side stream (it also primes the stream's scratch), the same call captured on it with the order given
    (one queue: the entry forks nothing), replayed twice on refilled buffers"""
    eng = engine()
    n = 129
    order = list(range(n - 1, -1, -1))
    cap = torch.cuda.Stream()

    if form == "pbkdf2":
        def make(seed):
            return kdf_case(n, 29, 2, seed, rot=0)                    # the same lengths, fresh octets

        pwds, raw, stride, salts = make(0)
        A = kdf_arena(pwds, raw, 29, stride, n, order=order, seed=31)

        def call():
            kdf_call(eng, A, 3, 29, stride, n)

        def load(seed):
            p, r, _, s = make(seed)
            A.put("pwds", b"".join(p))
            A.put("salts", r)
            return {"keys": b"".join(kdf(p[i], 3, s[i]) for i in range(n))}

        outputs = ["keys"]
        want0 = {"keys": b"".join(kdf(pwds[i], 3, salts[i]) for i in range(n))}
    else:
        shared = 33 if form == "write-shared" else None
        b = G.Batch(n, shared=shared, seed=20)
        verify = form == "verify"

        def wanted(x):
            if not verify:
                return {"macs": b"".join(x.want())}
            return {"codes": struct.pack(f"<{n}I", *spoil(x.want())[1])}

        A = hmac_arena(b, 32, macs=spoil(b.want())[0] if verify else None, order=order, seed=30)

        def call():
            hmac_call(eng, b, A, 32)

        def load(seed):
            x = G.Batch(n, shared=shared, seed=seed)                  # the same lengths, fresh octets
            assert x.msg_lens == b.msg_lens and x.key_lens == b.key_lens
            x.key = b.key                                             # (a shared key's state is baked into the captured launch)
            A.put("data", b"".join(x.msgs))
            if shared is None:
                A.put("keys", b"".join(x.keys))
            if verify:
                A.put("macs", b"".join(spoil(x.want())[0]))
            return wanted(x)

        outputs = ["codes"] if verify else ["macs"]
        want0 = wanted(b)

    torch.cuda.synchronize()
    with torch.cuda.stream(cap):
        call()
    cap.synchronize()
    assert A.fetch(outputs) == want0
    A.refill()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=cap):
        call()
    for seed in (41, 42):
        want = load(seed)
        A.refill()
        graph.replay()
        assert A.fetch(outputs) == want, seed


# ================================================================================================ host entries
def test_host_entries_equal_the_model():
    eng = engine()
    for b in (G.grid_batch(), G.batch(257, shared=42), G.batch(1)):
        key = b.keys if b.key is None else b.key
        want = b.want()
        assert eng.beltHMAC_ragged(key, b.msgs) == (0, want)
        assert eng.beltHMAC_ragged(key, b.msgs, 13) == (0, [m[:13] for m in want])
        macs, codes = spoil([m[:20] for m in want])
        assert eng.beltHMAC_verify_ragged(key, b.msgs, macs) == (0, codes)
    pwds, raw, stride, salts = kdf_case(65, 31, 1, 9)
    assert eng.beltPBKDF2_batch(pwds, 3, salts) == (0, [kdf(pwds[i], 3, salts[i]) for i in range(65)])
    assert eng.beltHMAC_ragged(b"k", []) == (0, []) and eng.beltPBKDF2_batch([], 1, b"salt") == (0, [])


def test_one_shots_on_the_host_and_through_the_kernel():
    """beltHMAC / beltPBKDF2: the host path by default, the kernel with n = 1 under path policy 1 (bee2hip_path_count says
    which ran), the host again above the iteration cap of a launch whatever the policy"""
    eng = engine()
    lib = eng.lib
    H = orclib.Golden().H
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "belt_hmac.json")))
    rnd = random.Random(77)
    cases = [(rnd.randbytes(k), rnd.randbytes(m)) for k, m in ((0, 0), (29, 32), (32, 1), (33, 100), (97, 1000), (5, 4101))]

    def count():
        return [lib.bee2hip_path_count(i) for i in range(3)]

    try:
        for policy, slot in ((0, 0), (1, 1), (2, 0)):
            lib.bee2hip_path_policy(policy)
            before = count()
            calls = 0
            for key, msg in cases:
                assert eng.beltHMAC(msg, key) == (0, M.hmac(key, msg)), (policy, len(key), len(msg))
                assert eng.beltPBKDF2(key, 3, msg) == (0, M.pbkdf2(key, 3, msg)), (policy, len(key), len(msg))
                calls += 2
            for v in fx["b1"]:
                assert eng.beltHMAC(H[192:224], H[128:128 + v["key_len"]])[1].hex() == v["mac"]
                calls += 1
            v = fx["pbkdf2"][1]
            assert eng.beltPBKDF2(v["pwd"].encode(), v["iter"], bytes.fromhex(v["salt"]))[1].hex() == v["key"]
            calls += 1
            after = count()
            assert after[slot] - before[slot] == calls and after[2] == before[2], (policy, before, after)
            assert after[1 - slot] == before[1 - slot], (policy, before, after)
        lib.bee2hip_path_policy(1)
        before = count()
        over = G.ITER_CAP + 1
        code, key = eng.beltPBKDF2(b"pwd", over, b"salt")
        after = count()
        assert code == 0 and after[0] == before[0] + 1 and after[1] == before[1]
    finally:
        lib.bee2hip_path_policy(0)
    # (the value of that many rounds is not recomputed here: the host path's rounds are held to the model on the CPU by
    # tests/test_belthmac.py; this is about which path ran)
    assert len(key) == 32 and any(key)


def test_smoke_vectors_as_record_1_of_3():
    """what smoke() runs: B.1-1 and the 10 000-iteration vector of the reference's tests"""
    eng, H = engine(), orclib.Golden().H
    code, macs = eng.beltHMAC_ragged([b"", H[128:157], bytes(33)], [b"a", H[192:224], b""])
    assert code == 0 and macs[1].hex().upper() == "D4828E6312B08BB83C9FA6535A4635549E411FD11C0D8289359A1130E930676B"
    code, keys = eng.beltPBKDF2_batch([b"", b"B194BAC80A08F53B", b"z" * 40], 10000, H[192:200])
    assert code == 0 and keys[1].hex().upper() == "3D331BBBB1FBBB40E4BF22F6CB9A689EF13A77DC09ECF93291BFE42439A72E7D"
