"""Rates of the belt-kwp batch on one GPU -> profiles/belt_kwp_rate.json.

  1. bee2hip_beltKWP_batch_stream, wrap and unwrap, in records/s at (wrap count x n) 32 x 2^20 and x 2^22, 16, 24, 19 (an
     unaligned tail) and 64 x 2^20, 1008 x 2^12 (a latency figure, not a rate); windows of at least 0.5 s, wrap and unwrap
     alternating, three repeats each (median)
  2. beside each: the reference (oracle/_ref/libbee2ref.so: beltKWPWrap / beltKWPUnwrap) through ctypes from 16 threads on a
     sample of the same records, outputs compared -- a floor for bee2.  The one hard condition: at 32 x 2^20 the batch is not
     slower than that sample, in both directions
  3. at 32 x 2^20: bee2hip_beltSDE_sectors_dev on the same number of 48-octet sectors -- the same belt-wbl on 48 octets plus two
     E_K, in the generic belt_sde_kernel -- the in-project yardstick
  4. --fold PARENT_LIB: bee2hip_beltDWP_absorb_dev on a 64 KiB and a 4 GiB message with the parent's library and with this one,
     each in a process of its own, three pairs with the order alternating (polyhash_prep_kernel and polyhash_finish_kernel were
     folded into one kernel); beside it, as a control, the generic belt_sde_kernel (48- and 528-octet sectors x 2^20, both
     directions), whose text is the parent's
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

SHAPES = ((32, 1 << 20), (32, 1 << 22), (16, 1 << 20), (24, 1 << 20), (19, 1 << 20), (64, 1 << 20), (1008, 1 << 12))
SDE_SECTORS = (48, 528)
ABSORB = (("64KiB", 64 << 10), ("4GiB", 4 << 30))


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


def gpu_part(out, shapes):
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
    key = bytes(range(32))
    kw = eng.beltKeyExpand2(key)
    _sz = ctypes.c_size_t
    out["shapes"] = []
    for count, n in shapes:
        T = count + 16
        g = torch.Generator(device="cuda").manual_seed(count + n)
        keys = torch.randint(0, 256, (n * count,), dtype=torch.uint8, device="cuda", generator=g)
        hdrs = torch.randint(0, 256, (n * 16,), dtype=torch.uint8, device="cuda", generator=g)
        tokens = torch.empty(n * T, dtype=torch.uint8, device="cuda")
        back = torch.empty_like(keys)
        codes = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        wrap = lambda: eng.beltKWP_batch_stream(0, key, hdrs, keys, count, n, tokens)
        unwrap = lambda: eng.beltKWP_batch_stream(1, key, hdrs, tokens, T, n, back, codes)
        sw, su = [], []
        for _ in range(3):
            sw.append(window(wrap, sync))
            su.append(window(unwrap, sync))
        assert torch.equal(back, keys) and not codes.any()
        e = {"count": count, "token_octets": T, "records": n, "wrap_records_per_s_runs": [n / s for s in sw],
             "unwrap_records_per_s_runs": [n / s for s in su], "wrap_records_per_s": n / med(sw), "unwrap_records_per_s": n / med(su),
             "wrap_ms": med(sw) * 1e3, "unwrap_ms": med(su) * 1e3}
        if ref is not None:
            sub = min(n, max(4096, (1 << 24) // T))
            hk, hh = keys[: sub * count].cpu().numpy().copy(), hdrs[: sub * 16].cpu().numpy().copy()
            ht, hb = np.empty(sub * T, dtype=np.uint8), np.empty(sub * count, dtype=np.uint8)
            bad = [0] * 16

            def work_wrap(t):
                for i in range(t, sub, 16):
                    bad[t] |= ref.beltKWPWrap(ctypes.c_void_p(ht.ctypes.data + T * i), ctypes.c_void_p(hk.ctypes.data + count * i),
                                              _sz(count), ctypes.c_void_p(hh.ctypes.data + 16 * i), key, _sz(32))

            def work_unwrap(t):
                for i in range(t, sub, 16):
                    bad[t] |= ref.beltKWPUnwrap(ctypes.c_void_p(hb.ctypes.data + count * i), ctypes.c_void_p(ht.ctypes.data + T * i),
                                                _sz(T), ctypes.c_void_p(hh.ctypes.data + 16 * i), key, _sz(32))
            dts = []
            for work in (work_wrap, work_unwrap):
                t0 = time.perf_counter()
                with ThreadPoolExecutor(16) as ex:
                    list(ex.map(work, range(16)))
                dts.append(time.perf_counter() - t0)
            same = bool((tokens[: sub * T].cpu().numpy() == ht).all()) and bool((hb == hk).all()) and not any(bad)
            e["cpu_reference"] = {"threads": 16, "sample_records": sub, "wrap_records_per_s": sub / dts[0],
                                  "unwrap_records_per_s": sub / dts[1], "outputs_equal": same,
                                  "wrap_over_reference": e["wrap_records_per_s"] / (sub / dts[0]),
                                  "unwrap_over_reference": e["unwrap_records_per_s"] / (sub / dts[1]),
                                  "note": "one foreign call per record from 16 Python threads is in the figure: a floor for bee2"}
            if (count, n) == (32, 1 << 20):
                e["cpu_reference"]["hard_condition_met"] = bool(same and e["cpu_reference"]["wrap_over_reference"] >= 1.0
                                                                and e["cpu_reference"]["unwrap_over_reference"] >= 1.0)
        if (count, n) == (32, 1 << 20):
            # the in-project yardstick: n sectors of 48 octets through the generic belt_sde_kernel (sector in HBM, rolling form)
            sec = torch.randint(0, 256, (n * 48,), dtype=torch.uint8, device="cuda", generator=g)
            sivs = torch.randint(0, 256, (n * 16,), dtype=torch.uint8, device="cuda", generator=g)
            se = [window(lambda: eng.beltSDE_sectors_dev(0, sec, 48, kw, sivs), sync) for _ in range(3)]
            sd = [window(lambda: eng.beltSDE_sectors_dev(1, sec, 48, kw, sivs), sync) for _ in range(3)]
            e["belt_sde_kernel_48"] = {"sectors_per_s_encr": n / med(se), "sectors_per_s_decr": n / med(sd),
                                       "wrap_over_sde_encr": e["wrap_records_per_s"] / (n / med(se)),
                                       "unwrap_over_sde_decr": e["unwrap_records_per_s"] / (n / med(sd))}
            del sec, sivs
        out["shapes"].append(e)
        print(json.dumps(e), flush=True)
        del keys, hdrs, tokens, back, codes


def fold_probe():
    """(a process of its own, the library chosen by BEE2HIP_LIB) -> one JSON line: ms per call of bee2hip_beltDWP_absorb_dev, whose
    two launches of polyhash_powers_kernel are the fold, and of the generic belt_sde_kernel, whose text is the parent's"""
    import torch
    import bee2_amd
    eng = bee2_amd.load()
    eng.set_device(0)
    sync = torch.cuda.synchronize
    H = eng.beltH()
    _, _, r, t0 = eng.beltDWPStart(H[128:160], H[192:208])
    g = torch.Generator(device="cuda").manual_seed(5)
    res = {}
    tout = torch.zeros(16, dtype=torch.uint8, device="cuda")
    for name, nbytes in ABSORB:
        buf = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=g)
        res[f"absorb_{name}_ms"] = 1e3 * window(lambda: eng.beltDWP_absorb_dev(buf, nbytes, r, t0, tout), sync)
        del buf
    kw = eng.beltKeyExpand2(bytes(range(32)))
    n = 1 << 20
    for sb in SDE_SECTORS:
        sec = torch.randint(0, 256, (n * sb,), dtype=torch.uint8, device="cuda", generator=g)
        sivs = torch.randint(0, 256, (n * 16,), dtype=torch.uint8, device="cuda", generator=g)
        for decr in (0, 1):
            res[f"sde_{'decr' if decr else 'encr'}_{sb}_ms"] = 1e3 * window(lambda: eng.beltSDE_sectors_dev(decr, sec, sb, kw, sivs), sync)
        del sec, sivs
    print(json.dumps(res))


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

    def legs(prefix):
        res = {}
        for k in sorted(runs["this"][0]):
            if k.startswith(prefix):
                p, t = [r[k] for r in runs["parent"]], [r[k] for r in runs["this"]]
                res[k] = {"parent_median": med(p), "this_median": med(t), "parent_spread": max(p) - min(p), "this_over_parent": med(t) / med(p),
                          "medians_differ_by": abs(med(t) - med(p)), "within_parent_spread": abs(med(t) - med(p)) <= max(p) - min(p)}
        return res
    rec = {"what": "ms per call of bee2hip_beltDWP_absorb_dev on a resident message: polyhash_powers_kernel (one kernel, launched before and "
                   "after polyhash_kernel, the step an argument) against the parent's polyhash_prep_kernel and polyhash_finish_kernel; each "
                   "library in processes of its own, three pairs, order alternating",
           "criterion": "medians differ by no more than the parent's own spread", "runs": runs, "legs": legs("absorb_"),
           "control_unchanged_kernel": {"what": "ms per call, 2^20 sectors, belt_sde_kernel<0> / <1>: the same text in both libraries, so what "
                                                "two builds of one kernel differ by in this session", "legs": legs("sde_")},
           "bench_legs": "the belt_dwp leg of bench.py --all calls bee2hip_beltDWP_absorb_dev on a 4 GiB message: absorb_4GiB_ms is its mac_only "
                         "figure's shape; no BASELINE leg launches the kernel"}
    rec["criterion_met"] = all(v["within_parent_spread"] for v in rec["legs"].values())
    out["fold_non_regression"] = rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "belt_kwp_rate.json"))
    ap.add_argument("--fold", metavar="PARENT_LIB", default=None, help="libbee2hip.so built from the parent commit")
    ap.add_argument("--skip-rates", action="store_true")
    ap.add_argument("--fold-probe", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.fold_probe:
        return fold_probe()
    out = {}
    if os.path.exists(args.out):
        out = json.load(open(args.out))
    if args.fold:                       # first: the probes run in processes of their own, before this one opens the GPU
        fold_part(out, args.fold)
    if not args.skip_rates:
        gpu_part(out, SHAPES)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
