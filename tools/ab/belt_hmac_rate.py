"""Rates of the belt-hmac / belt-pbkdf2 batches on one GPU -> profiles/belt_hmac_rate.json.

  1. bee2hip_beltHMAC_ragged_stream at 2^18 x 64 and 2^18 x 1000 octets, and at 2^14 x 1000 (the batch size at which the ragged
     belt-hash still runs its 4 KiB-table form), with one shared key and with 32-octet keys per record; windows of at least
     0.5 s, three repeats (median); time per belt-compress = time / (n x compressions of a record)
  2. the yardstick: bee2hip_hash_ragged_dev(alg = 0) on the same 1000-octet batches: 33 compressions a message (HMAC: 35 with a
     shared key, 37 with its own), and which table form that launch uses at that n
  3. bee2hip_beltPBKDF2_batch_stream: 2^16 passwords at 10 000 iterations (4 compressions an iteration); launches of 64
     passwords at 2^14 and 2^16 iterations and at the cap of a launch, 2^17 ("proposed_cap_2_20" in the record is the same
     launch at 2^20, the cap first proposed, measured before it was lowered)
  4. beside each: the reference (oracle/_ref/libbee2ref.so: beltHMAC / beltPBKDF2) through ctypes from 16 threads on a sample of
     the same records, outputs compared -- a floor for bee2
  5. --fold PARENT_LIB: bee2hip_bashHash_beltMAC_batch_dev at msg_len 100, n = 2^16 (the generic path, whose two one-thread-per-item
     helper kernels became one) with the parent's library and with this one, each in a process of its own, three pairs with the
     order alternating
  6. the kernel's registers, scratch and code size, read off the built library (no GPU)
Batches are device-resident and warmed up; a timed window ends in a synchronise."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

HMAC_SHAPES = ((64, 1 << 18), (1000, 1 << 18), (1000, 1 << 14))
KERNEL = "belt_hmac_batch_kernel"


def window(fn, sync, least=0.5):
    """seconds per call over a window of at least `least` seconds"""
    fn()
    sync()
    reps = 1
    while True:
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        sync()
        dt = time.perf_counter() - t0
        if dt >= least:
            return dt / reps
        reps = max(2 * reps, int(reps * 1.2 * least / max(dt, 1e-6)) + 1)


def med(v):
    return sorted(v)[len(v) // 2]


def blocks(octets):
    return (octets + 31) // 32


def meta_part(out):
    import kernel_meta
    import bee2_amd
    lib = bee2_amd.LIB_PATH
    k = [x for x in kernel_meta.kernels(lib) if KERNEL in x["name"]]
    assert len(k) == 1, k
    tmp = subprocess.check_output(["mktemp", "-d"], text=True).strip()
    subprocess.check_call(["cp", os.path.realpath(lib), os.path.join(tmp, "lib.so")])
    subprocess.run([f"{kernel_meta.LLVM}/llvm-objdump", "--offloading", "lib.so"], cwd=tmp, capture_output=True)
    size = None
    for co in sorted(os.listdir(tmp)):
        if "gfx950" in co:
            syms = subprocess.check_output([f"{kernel_meta.LLVM}/llvm-readelf", "-s", "-W", os.path.join(tmp, co)], text=True)
            for line in syms.splitlines():
                f = line.split()
                if len(f) >= 8 and f[3] == "FUNC" and KERNEL in f[7]:
                    size = int(f[2])
    subprocess.call(["rm", "-rf", tmp])
    out["kernel"] = {"name": k[0]["name"], "vgpr": int(k[0]["vgpr"]), "sgpr": int(k[0]["sgpr"]), "scratch": int(k[0]["scratch"]),
                     "vgpr_spills": int(k[0]["spill"]), "static_lds": int(k[0]["lds"]), "code_bytes": size,
                     "belt_compress_sites": 2, "note": "one site in the absorbing loop (key, pads, message, closing blocks, outer "
                     "hash), one in the iteration loop; code_bytes is the size of the kernel's symbol, against a 64 KiB instruction cache"}
    print(json.dumps(out["kernel"]), flush=True)


def gpu_part(out, parts):
    import numpy as np
    import torch
    import bee2_amd
    import refgen
    from concurrent.futures import ThreadPoolExecutor
    eng = bee2_amd.load()
    eng.set_device(0)
    sync = torch.cuda.synchronize
    out["device"] = torch.cuda.get_device_name(0)
    out["engine"] = eng.version()
    ref = ctypes.CDLL(refgen.REF_SO) if refgen.have_ref() else None
    _sz = ctypes.c_size_t
    key = bytes(range(32))
    cus = torch.cuda.get_device_properties(0).multi_processor_count

    def threads16(work):
        t0 = time.perf_counter()
        with ThreadPoolExecutor(16) as ex:
            list(ex.map(work, range(16)))
        return time.perf_counter() - t0

    if "hmac" in parts:
        out["hmac"] = []
    for mlen, n in HMAC_SHAPES if "hmac" in parts else ():
        g = torch.Generator(device="cuda").manual_seed(mlen + n)
        data = torch.randint(0, 256, (n * mlen,), dtype=torch.uint8, device="cuda", generator=g)
        offs = torch.arange(0, (n + 1) * mlen, mlen, dtype=torch.int64, device="cuda")
        keys = torch.randint(0, 256, (n * 32,), dtype=torch.uint8, device="cuda", generator=g)
        koffs = torch.arange(0, (n + 1) * 32, 32, dtype=torch.int64, device="cuda")
        macs, macs2 = torch.empty(n * 32, dtype=torch.uint8, device="cuda"), torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        codes = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        shared = lambda: eng.beltHMAC_ragged_stream(0, key, None, None, data, offs, None, n, macs, 32)
        own = lambda: eng.beltHMAC_ragged_stream(0, None, keys, koffs, data, offs, None, n, macs2, 32)
        ss, so = [], []
        for _ in range(3):
            ss.append(window(shared, sync))
            so.append(window(own, sync))
        eng.beltHMAC_ragged_stream(1, key, None, None, data, offs, None, n, macs, 32, codes)
        sync()
        assert not codes.any()
        cs, co = blocks(mlen) + 3, blocks(mlen) + 5                # + closing, 2 outer / + the two pad blocks
        e = {"msg_octets": mlen, "records": n, "shared_key_ms_runs": [1e3 * s for s in ss], "own_keys_ms_runs": [1e3 * s for s in so],
             "shared_key_ms": 1e3 * med(ss), "own_keys_ms": 1e3 * med(so), "shared_key_macs_per_s": n / med(ss),
             "own_keys_macs_per_s": n / med(so), "compressions_shared": cs, "compressions_own": co,
             "ns_per_compression_shared": 1e9 * med(ss) / (n * cs), "ns_per_compression_own": 1e9 * med(so) / (n * co),
             "ns_per_compression_shared_spread": 1e9 * (max(ss) - min(ss)) / (n * cs)}
        if mlen == 1000:
            dig = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
            sh = [window(lambda: eng.hash_ragged_dev(0, data, offs, dig, n), sync) for _ in range(3)]
            ch = blocks(mlen) + 1
            form = "BeltTabSmall (4 KiB), 64-thread workgroups" if n < 32768 else \
                ("BeltTabTwoP (64 KiB), 1024-thread workgroups" if n >= cus * 1024 else "BeltTabTwoP (64 KiB), 256-thread workgroups")
            e["belt_hash_ragged"] = {"ms_runs": [1e3 * s for s in sh], "ms": 1e3 * med(sh), "compressions": ch, "table_form": form,
                                     "same_table_as_hmac": n < 32768, "ns_per_compression": 1e9 * med(sh) / (n * ch),
                                     "ns_per_compression_spread": 1e9 * (max(sh) - min(sh)) / (n * ch),
                                     "hmac_shared_over_hash_per_compression": (med(ss) / cs) / (med(sh) / ch),
                                     "hmac_own_over_hash_per_compression": (med(so) / co) / (med(sh) / ch)}
            del dig
        if ref is not None:
            sub = min(n, max(4096, (1 << 23) // max(mlen, 32)))
            hd, hk = data[: sub * mlen].cpu().numpy().copy(), keys[: sub * 32].cpu().numpy().copy()
            hm = np.empty(sub * 32, dtype=np.uint8)
            bad = [0] * 16

            def work(t):
                for i in range(t, sub, 16):
                    bad[t] |= ref.beltHMAC(ctypes.c_void_p(hm.ctypes.data + 32 * i), ctypes.c_void_p(hd.ctypes.data + mlen * i), _sz(mlen),
                                           ctypes.c_void_p(hk.ctypes.data + 32 * i), _sz(32))
            dt = threads16(work)
            same = bool((macs2[: sub * 32].cpu().numpy() == hm).all()) and not any(bad)
            e["cpu_reference"] = {"threads": 16, "sample_records": sub, "macs_per_s": sub / dt, "outputs_equal": same,
                                  "own_keys_over_reference": e["own_keys_macs_per_s"] / (sub / dt),
                                  "note": "one foreign call per record from 16 Python threads is in the figure: a floor for bee2"}
        out["hmac"].append(e)
        print(json.dumps(e), flush=True)
        del data, offs, keys, koffs, macs, macs2, codes

    # ---- PBKDF2
    n, it = 1 << 16, 10000
    g = torch.Generator(device="cuda").manual_seed(7)
    pwds = torch.randint(0, 256, (n * 16,), dtype=torch.uint8, device="cuda", generator=g)
    poffs = torch.arange(0, (n + 1) * 16, 16, dtype=torch.int64, device="cuda")
    salts = torch.randint(0, 256, (n * 8,), dtype=torch.uint8, device="cuda", generator=g)
    dks = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    if "pbkdf2" in parts:
        pbkdf2_rate(out, eng, sync, ref, threads16, n, it, pwds, poffs, salts, dks)
    if "cap" in parts:
        pbkdf2_cap(out, eng, sync, pwds, poffs, salts, dks)


def pbkdf2_rate(out, eng, sync, ref, threads16, n, it, pwds, poffs, salts, dks):
    import numpy as np
    _sz = ctypes.c_size_t
    runs = [window(lambda: eng.beltPBKDF2_batch_stream(pwds, poffs, it, salts, 8, 8, None, n, dks), sync) for _ in range(3)]
    comp = 4 * it + 3                                                # two pads, one salt block, closing, two outer; then 4 a round
    p = {"passwords": n, "iter": it, "pwd_octets": 16, "salt_octets": 8, "s_runs": runs, "s": med(runs), "keys_per_s": n / med(runs),
         "compressions": comp, "ns_per_compression": 1e9 * med(runs) / (n * comp)}
    if ref is not None:
        sub = 256
        hp, hs = pwds[: sub * 16].cpu().numpy().copy(), salts[: sub * 8].cpu().numpy().copy()
        hk = np.empty(sub * 32, dtype=np.uint8)
        bad = [0] * 16

        def work(t):
            for i in range(t, sub, 16):
                bad[t] |= ref.beltPBKDF2(ctypes.c_void_p(hk.ctypes.data + 32 * i), ctypes.c_void_p(hp.ctypes.data + 16 * i), _sz(16), _sz(it),
                                         ctypes.c_void_p(hs.ctypes.data + 8 * i), _sz(8))
        dt = threads16(work)
        same = bool((dks[: sub * 32].cpu().numpy() == hk).all()) and not any(bad)
        p["cpu_reference"] = {"threads": 16, "sample_records": sub, "keys_per_s": sub / dt, "outputs_equal": same,
                              "batch_over_reference": p["keys_per_s"] / (sub / dt)}
    out["pbkdf2"] = p
    print(json.dumps(p), flush=True)


def pbkdf2_cap(out, eng, sync, pwds, poffs, salts, dks):
    """one wavefront's worth of passwords: what an iteration costs a launch in wall time, and the cap itself"""
    n, cap = 64, 1 << 17
    lone = []
    for its in (1 << 14, 1 << 16, cap):
        t0 = time.perf_counter()
        eng.beltPBKDF2_batch_stream(pwds, poffs, its, salts, 8, 8, None, n, dks)
        sync()
        lone.append({"iter": its, "s": time.perf_counter() - t0})
    per_iter = (lone[1]["s"] - lone[0]["s"]) / (lone[1]["iter"] - lone[0]["iter"])
    c = dict(out.get("pbkdf2_cap", {}))
    c.update({"passwords": n, "launches": lone, "s_per_iteration": per_iter, "cap_iter": cap, "cap_launch_s": lone[2]["s"]})
    out["pbkdf2_cap"] = c
    print(json.dumps(c), flush=True)


def fold_probe():
    """(a process of its own, the library chosen by BEE2HIP_LIB) -> one JSON line: ms per call of bee2hip_bashHash_beltMAC_batch_dev on
    the generic path (msg_len 100 is no multiple of 16)"""
    import torch
    import bee2_amd
    eng = bee2_amd.load()
    eng.set_device(0)
    sync = torch.cuda.synchronize
    n, mlen = 1 << 16, 100
    g = torch.Generator(device="cuda").manual_seed(5)
    msgs = torch.randint(0, 256, (n * mlen,), dtype=torch.uint8, device="cuda", generator=g)
    dig = torch.empty(n * 64, dtype=torch.uint8, device="cuda")
    tag = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
    runs = [1e3 * window(lambda: eng.bashHash_beltMAC_batch_dev(msgs, mlen, 256, bytes(range(32)), dig, tag, n), sync) for _ in range(3)]
    print(json.dumps({"mixed_100_ms": med(runs), "mixed_100_ms_runs": runs,
                      "sum": int(dig.sum().item()) + int(tag.sum().item())}))


def fold_part(out, parent_lib):
    runs = {"parent": [], "this": []}
    for rnd in range(3):
        for which in (("parent", "this") if rnd % 2 == 0 else ("this", "parent")):
            env = dict(os.environ)
            if which == "parent":
                env["BEE2HIP_LIB"] = os.path.abspath(parent_lib)
            else:
                env.pop("BEE2HIP_LIB", None)
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--fold-probe"], cwd=ROOT, env=env, check=True, timeout=240,
                                 stdout=subprocess.PIPE, text=True)
            runs[which].append(json.loads(run.stdout.strip().splitlines()[-1]))
            print(which, runs[which][-1], flush=True)
    p, t = [r["mixed_100_ms"] for r in runs["parent"]], [r["mixed_100_ms"] for r in runs["this"]]
    assert len({r["sum"] for r in runs["parent"] + runs["this"]}) == 1, "the two libraries computed different results"
    out["helper_kernel_fold"] = {
        "what": "ms per call of bee2hip_bashHash_beltMAC_batch_dev, msg_len 100, n = 2^16, l = 256 (the generic path): mixed_states_kernel "
                "(one kernel, launched before and after the two byte-granular kernels, the direction an argument) against the parent's "
                "init_states_kernel and gather_results_kernel; each library in processes of its own, three pairs, order alternating",
        "criterion": "the new median lies inside the parent's spread (its runs' minimum .. maximum)", "runs": runs,
        "parent_median": med(p), "this_median": med(t), "parent_min": min(p), "parent_max": max(p), "this_over_parent": med(t) / med(p),
        "criterion_met": min(p) <= med(t) <= max(p)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "belt_hmac_rate.json"))
    ap.add_argument("--fold", metavar="PARENT_LIB", default=None, help="libbee2hip.so built from the parent commit")
    ap.add_argument("--parts", default="hmac,pbkdf2,cap", help="which of hmac, pbkdf2, cap to measure ('' = none)")
    ap.add_argument("--fold-probe", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.fold_probe:
        return fold_probe()
    out = {}
    if os.path.exists(args.out):
        out = json.load(open(args.out))
    meta_part(out)
    if args.fold:                       # first: the probes run in processes of their own, before this one opens the GPU
        fold_part(out, args.fold)
    parts = [x for x in args.parts.split(",") if x]
    if parts:
        gpu_part(out, parts)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
