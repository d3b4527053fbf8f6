"""The bpki container batches and the per-record-key belt-kwp on one GPU -> profiles/bpki_rate.json.

  1. --parent PARENT_LIB: the shared-key path must not pay for the key argument of belt_kwp_batch_kernel.  The legs of
     tools/ab/belt_kwp_rate.py (bee2hip_beltKWP_batch_stream, wrap and unwrap, every shape there) with the parent's library and
     with this one, each in a process of its own, --pairs pairs (default three) with the order alternating.  Criterion: this build's
     median lies inside the spread of the parent's own runs (min .. max), leg by leg.  The same processes time
     bee2hip_hash_ragged_dev on 2^16 x 100 octets, whose ragged_order_kernel is the fold that paid for the keyed instantiation.
  2. the keyed form next to the shared-key one: ms per call and tokens/s at T = 81 and T = 1024, n = 2^18, both directions.
  3. end to end: bee2hip_bpkiUnwrap_batch on 2^16 private-key containers (32-octet keys, 10000 iterations, sealed by
     bee2hip_bpkiWrap_batch): wall time of the call, containers/s, and beside it the two device steps on the same records on
     their own (bee2hip_beltPBKDF2_batch_stream, bee2hip_beltKWP_keyed_batch_stream) -- the kwp launch's share of the call.
     Yardstick: the reference's bpkiPrivkeyUnwrap (oracle/_ref/libbee2ref.so) through ctypes from 16 threads on 256 of the
     same containers, keys compared.
Batches are device-resident and warmed up where the entry takes device pointers; a timed window ends in a synchronise."""
import argparse
import ctypes
import json
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools"), os.path.join(ROOT, "tools", "ab")]
from belt_kwp_rate import SHAPES, med, window  # noqa: E402

_sz, _u32, _u64 = ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64


def shared_probe():
    """(a process of its own, the library chosen by BEE2HIP_LIB) -> one JSON line: ms per call of the shared-key entry"""
    import torch
    import bee2_amd
    eng = bee2_amd.load()
    eng.set_device(0)
    sync = torch.cuda.synchronize
    key, res = bytes(range(32)), {}
    for count, n in SHAPES:
        T = count + 16
        g = torch.Generator(device="cuda").manual_seed(count + n)
        keys = torch.randint(0, 256, (n * count,), dtype=torch.uint8, device="cuda", generator=g)
        hdrs = torch.randint(0, 256, (n * 16,), dtype=torch.uint8, device="cuda", generator=g)
        tokens = torch.empty(n * T, dtype=torch.uint8, device="cuda")
        back = torch.empty_like(keys)
        codes = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        res[f"wrap_{count}x{n}_ms"] = 1e3 * window(lambda: eng.beltKWP_batch_stream(0, key, hdrs, keys, count, n, tokens), sync)
        res[f"unwrap_{count}x{n}_ms"] = 1e3 * window(lambda: eng.beltKWP_batch_stream(1, key, hdrs, tokens, T, n, back, codes), sync)
        assert torch.equal(back, keys) and not codes.any()
        del keys, hdrs, tokens, back, codes
    # the fold that paid for the keyed instantiation: ragged_order_kernel (was ragged_hist_kernel + ragged_scatter_kernel) orders
    # the records of bee2hip_hash_ragged_dev; belt-hash and bash256 of 2^16 messages of 100 octets
    n = 1 << 16
    g = torch.Generator(device="cuda").manual_seed(100)
    data = torch.randint(0, 256, (n * 100,), dtype=torch.uint8, device="cuda", generator=g)
    offs = torch.arange(0, (n + 1) * 100, 100, dtype=torch.int64, device="cuda")
    dig = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    for alg in (0, 128):
        res[f"hash_ragged_alg{alg}_65536x100_ms"] = 1e3 * window(lambda: eng.hash_ragged_dev(alg, data, offs, dig, n), sync)
    print(json.dumps(res))


def shared_part(out, parent_lib, pairs):
    runs = {"parent": [], "this": []}
    for rnd in range(pairs):
        for which in (("parent", "this") if rnd % 2 == 0 else ("this", "parent")):
            env = dict(os.environ)
            if which == "parent":
                env["BEE2HIP_LIB"] = os.path.abspath(parent_lib)
            else:
                env.pop("BEE2HIP_LIB", None)
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--shared-probe"], cwd=ROOT, env=env, check=True, timeout=240,
                                 stdout=subprocess.PIPE, text=True)
            runs[which].append(json.loads(run.stdout.strip().splitlines()[-1]))
            print(which, runs[which][-1], flush=True)
    legs = {}
    for k in sorted(runs["this"][0]):
        p, t = [r[k] for r in runs["parent"]], [r[k] for r in runs["this"]]
        legs[k] = {"parent_runs": p, "this_runs": t, "parent_median": med(p), "this_median": med(t), "this_over_parent": med(t) / med(p),
                   "inside_parent_spread": min(p) <= med(t) <= max(p), "not_slower_than_parent_max": med(t) <= max(p)}
    kwp = {k: v for k, v in legs.items() if "wrap" in k}
    fold = {k: v for k, v in legs.items() if k.startswith("hash_ragged")}
    out["shared_key_non_regression"] = {
        "what": "ms per call of bee2hip_beltKWP_batch_stream: belt_kwp_batch_kernel<false>, the shared-key instantiation, whose text is "
                "the parent's kernel (the keyed form is belt_kwp_batch_kernel<true>); each library in processes of its own, `pairs` pairs, "
                "order alternating",
        "pairs": pairs, "criterion": "this build's median inside the spread (min .. max) of the parent's own runs",
        "legs": kwp,
        "criterion_met": all(v["inside_parent_spread"] for v in kwp.values()),
        "no_leg_slower_than_the_parent_slowest_run": all(v["not_slower_than_parent_max"] for v in kwp.values())}
    out["ragged_order_fold_non_regression"] = {
        "what": "ms per call of bee2hip_hash_ragged_dev on 2^16 messages of 100 octets (alg 0 = belt-hash, 128 = bash256): the launch order "
                "comes from ragged_order_kernel, one kernel launched twice with a phase argument, against the parent's ragged_hist_kernel "
                "and ragged_scatter_kernel; same processes and pairs as above",
        "pairs": pairs, "criterion": "this build's median inside the spread (min .. max) of the parent's own runs",
        "legs": fold, "criterion_met": all(v["inside_parent_spread"] for v in fold.values()),
        "no_leg_slower_than_the_parent_slowest_run": all(v["not_slower_than_parent_max"] for v in fold.values())}


def keyed_part(out, eng, torch):
    sync = torch.cuda.synchronize
    n, key, rows = 1 << 18, bytes(range(32)), []
    for T in (81, 1024):
        count = T - 16
        g = torch.Generator(device="cuda").manual_seed(T)
        recs = torch.randint(0, 256, (n * count,), dtype=torch.uint8, device="cuda", generator=g)
        hdrs = torch.randint(0, 256, (n * 16,), dtype=torch.uint8, device="cuda", generator=g)
        keks = torch.randint(0, 256, (n * 32,), dtype=torch.uint8, device="cuda", generator=g)
        tokens, back = torch.empty(n * T, dtype=torch.uint8, device="cuda"), torch.empty_like(recs)
        codes = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        legs = {"keyed_wrap": lambda: eng.beltKWP_keyed_batch_stream(0, keks, 32, hdrs, recs, count, n, tokens),
                "keyed_unwrap": lambda: eng.beltKWP_keyed_batch_stream(1, keks, 32, hdrs, tokens, T, n, back, codes)}
        e = {"token_octets": T, "records": n}
        for name, fn in legs.items():
            s = [window(fn, sync) for _ in range(3)]
            e[name + "_ms"], e[name + "_tokens_per_s"] = 1e3 * med(s), n / med(s)
        assert torch.equal(back, recs) and not codes.any()
        legs = {"shared_wrap": lambda: eng.beltKWP_batch_stream(0, key, hdrs, recs, count, n, tokens),
                "shared_unwrap": lambda: eng.beltKWP_batch_stream(1, key, hdrs, tokens, T, n, back, codes)}
        for name, fn in legs.items():
            s = [window(fn, sync) for _ in range(3)]
            e[name + "_ms"], e[name + "_tokens_per_s"] = 1e3 * med(s), n / med(s)
        assert torch.equal(back, recs) and not codes.any()
        e["keyed_over_shared_wrap_ms"] = e["keyed_wrap_ms"] / e["shared_wrap_ms"]
        e["keyed_over_shared_unwrap_ms"] = e["keyed_unwrap_ms"] / e["shared_unwrap_ms"]
        rows.append(e)
        print(json.dumps(e), flush=True)
        del recs, hdrs, keks, tokens, back, codes
    out["keyed_next_to_shared"] = rows


def end_to_end(out, eng, torch):
    import numpy as np
    import refgen
    from concurrent.futures import ThreadPoolExecutor
    n, iters = 1 << 16, 10000
    rnd = random.Random(78)
    keys, salts = rnd.randbytes(32 * n), rnd.randbytes(8 * n)
    pwds = [rnd.randbytes(8 + i % 17) for i in range(n)]
    poffs = [0]
    for p in pwds:
        poffs.append(poffs[-1] + len(p))
    pdata, poff = b"".join(pwds), (_u64 * (n + 1))(*poffs)
    L = _sz(0)
    lib = eng.lib
    assert lib.bee2hip_bpkiWrap_batch(0, keys, _sz(32), pdata, poff, salts, _sz(iters), _sz(n), None, ctypes.byref(L)) == 0
    epkis = ctypes.create_string_buffer(n * L.value)
    t0 = time.perf_counter()
    assert lib.bee2hip_bpkiWrap_batch(0, keys, _sz(32), pdata, poff, salts, _sz(iters), _sz(n), epkis, ctypes.byref(L)) == 0
    wrap_s = time.perf_counter() - t0
    eoff = (_u64 * (n + 1))(*[L.value * i for i in range(n + 1)])
    got, lens, codes = ctypes.create_string_buffer(64 * n), (_u32 * n)(), (_u32 * n)()
    walls = []
    for _ in range(4):                                                  # (the first call grows the staging: not counted)
        t0 = time.perf_counter()
        assert lib.bee2hip_bpkiUnwrap_batch(0, epkis, eoff, pdata, poff, _sz(n), got, lens, codes) == 0
        walls.append(time.perf_counter() - t0)
    raw = np.frombuffer(got.raw, dtype=np.uint8).reshape(n, 64)
    assert not any(codes) and set(lens) == {32} and raw[:, :32].tobytes() == keys and not raw[:, 32:].any()
    wall = med(walls[1:])
    # the two device steps on their own, on the same records
    sync = torch.cuda.synchronize
    T = 81
    d_pw = torch.from_numpy(np.frombuffer(pdata, dtype=np.uint8).copy()).cuda()
    d_off = torch.from_numpy(np.array(poffs, dtype=np.int64)).cuda()
    d_salt = torch.from_numpy(np.frombuffer(salts, dtype=np.uint8).copy()).cuda()
    d_kek = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
    e = np.frombuffer(epkis.raw, dtype=np.uint8).reshape(n, L.value)
    d_tok = torch.from_numpy(e[:, L.value - T:].copy().reshape(-1)).cuda()
    d_out, d_codes = torch.empty(n * (T - 16), dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    kdf = med([window(lambda: eng.beltPBKDF2_batch_stream(d_pw, d_off, iters, d_salt, 8, 8, None, n, d_kek), sync, least=0.2) for _ in range(3)])
    kwp = med([window(lambda: eng.beltKWP_keyed_batch_stream(1, d_kek, 32, None, d_tok, T, n, d_out, d_codes), sync, least=0.2) for _ in range(3)])
    assert not d_codes.any()
    rec = {"what": "bee2hip_bpkiUnwrap_batch on 2^16 private-key containers (32-octet keys, 10000 iterations, passwords of 8 .. 24 octets), "
                   "host pointers in and out; median of three calls after a first one",
           "containers": n, "container_octets": L.value, "unwrap_wall_s_runs": walls[1:], "unwrap_wall_s": wall, "containers_per_s": n / wall,
           "wrap_wall_s_first_call": wrap_s, "pbkdf2_launch_s": kdf, "kwp_launch_s": kwp, "kwp_share_of_wall": kwp / wall,
           "pbkdf2_share_of_wall": kdf / wall, "host_and_copies_s": wall - kdf - kwp}
    if refgen.have_ref():
        ref = ctypes.CDLL(refgen.REF_SO)
        sub, outs, bad = 256, [ctypes.create_string_buffer(64) for _ in range(256)], [0] * 16
        head = epkis.raw[:L.value * sub]
        conts = [head[L.value * i:L.value * (i + 1)] for i in range(sub)]

        def work(t):
            for i in range(t, sub, 16):
                m = _sz(0)
                bad[t] |= ref.bpkiPrivkeyUnwrap(outs[i], ctypes.byref(m), conts[i], _sz(L.value), pwds[i], _sz(len(pwds[i])))
        t0 = time.perf_counter()
        with ThreadPoolExecutor(16) as ex:
            list(ex.map(work, range(16)))
        dt = time.perf_counter() - t0
        same = not any(bad) and all(outs[i].raw[:32] == keys[32 * i:32 * i + 32] for i in range(sub))
        rec["cpu_reference"] = {"threads": 16, "sample_containers": sub, "containers_per_s": sub / dt, "keys_equal": bool(same),
                                "batch_over_reference": (n / wall) / (sub / dt),
                                "note": "bpkiPrivkeyUnwrap through ctypes from 16 Python threads (the call releases the GIL)"}
    out["end_to_end"] = rec
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bpki_rate.json"))
    ap.add_argument("--parent", metavar="PARENT_LIB", default=None, help="libbee2hip.so built from the parent commit")
    ap.add_argument("--pairs", type=int, default=3, help="pairs of processes of the --parent comparison (odd: the median is a run)")
    ap.add_argument("--shared-probe", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.shared_probe:
        return shared_probe()
    out = {}                            # (nothing is carried over from an earlier file: every section comes from this run)
    if args.parent:                     # first: the probes run in processes of their own, before this one opens the GPU
        shared_part(out, args.parent, args.pairs)
    import torch
    import bee2_amd
    eng = bee2_amd.load()
    eng.set_device(0)
    out["device"], out["engine"] = torch.cuda.get_device_name(0), eng.version()
    keyed_part(out, eng, torch)
    end_to_end(out, eng, torch)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
