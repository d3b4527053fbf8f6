"""Rates of the belt-fmt record batch on one GPU -> profiles/belt_fmt_rate.json.

  1. bee2hip_beltFMT_batch_stream, encrypt and decrypt, in records/s: (10, 16) at 2^20 and 2^22 records, (58, 21) and (36, 50) at
     2^20, (65536, 32) at 2^18, (65536, 600) at 2^12; windows of at least 0.5 s, encrypt and decrypt alternating, three repeats
     each (median)
  2. beside each: the reference (oracle/_ref/libbee2ref.so: beltFMTEncr) through ctypes from 16 threads on a sample of the same
     records, outputs compared -- a floor for bee2 -- and belt_cbc_encr_kernel (bee2hip_beltCBCEncr_batch_dev) on the same
     number of messages of 6 blocks: one lane per message and six chained E_K, the E_K-only yardstick
  3. --fold PARENT_LIB: `bench.py --full` with the parent's library and with this one, three times each; --mirrored: the same
     with the order inside the pairs turned round (belt_encr_blocks_kernel and belt_decr_blocks_kernel were folded into one)
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

SHAPES = ((10, 16, 1 << 20), (10, 16, 1 << 22), (58, 21, 1 << 20), (36, 50, 1 << 20), (65536, 32, 1 << 18), (65536, 600, 1 << 12))


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


def gpu_part(out, shapes, with_ref=True):
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
    ref = ctypes.CDLL(refgen.REF_SO) if with_ref and refgen.have_ref() else None
    key = bytes(range(32))
    kw = eng.beltKeyExpand2(key)
    _sz = ctypes.c_size_t
    med = lambda v: sorted(v)[len(v) // 2]
    out["shapes"] = []
    for mod, count, n in shapes:
        g = torch.Generator(device="cuda").manual_seed(mod + count)
        data = torch.randint(0, mod, (n * count,), dtype=torch.int32, device="cuda", generator=g).to(torch.int16).view(torch.uint8)
        ivs = torch.randint(0, 256, (n * 16,), dtype=torch.uint8, device="cuda", generator=g)
        ct, pt = torch.empty_like(data), torch.empty_like(data)
        encr = lambda: eng.beltFMT_batch_stream(0, mod, count, key, ivs, data, ct, n)
        decr = lambda: eng.beltFMT_batch_stream(1, mod, count, key, ivs, ct, pt, n)
        se, sd = [], []
        for _ in range(3):
            se.append(window(encr, sync))
            sd.append(window(decr, sync))
        assert torch.equal(pt, data) and not torch.equal(ct, data)
        e = {"mod": mod, "count": count, "records": n, "encr_records_per_s_runs": [n / s for s in se],
             "decr_records_per_s_runs": [n / s for s in sd], "encr_records_per_s": n / med(se), "decr_records_per_s": n / med(sd),
             "encr_ms": med(se) * 1e3}
        if ref is not None:
            sub = min(n, max(256, (1 << 22) // count))
            src = data[: sub * count * 2].cpu().numpy().copy()
            host = np.empty_like(src)
            hiv = ivs[: sub * 16].cpu().numpy().copy()

            def work(r):
                for i in r:
                    ref.beltFMTEncr(ctypes.c_void_p(host.ctypes.data + 2 * count * i), ctypes.c_uint32(mod),
                                    ctypes.c_void_p(src.ctypes.data + 2 * count * i), _sz(count), key, _sz(32),
                                    ctypes.c_void_p(hiv.ctypes.data + 16 * i))
            t0 = time.perf_counter()
            with ThreadPoolExecutor(16) as ex:
                list(ex.map(work, [range(t, sub, 16) for t in range(16)]))
            dt = time.perf_counter() - t0
            same = bool((ct[: sub * count * 2].cpu().numpy() == host).all())
            e["cpu_reference"] = {"threads": 16, "sample_records": sub, "encr_records_per_s": sub / dt, "outputs_equal": same,
                                  "batch_over_reference": (n / med(se)) / (sub / dt),
                                  "note": "one foreign call per record from 16 Python threads is in the figure: a floor for bee2"}
        # the E_K-only yardstick: n messages of 6 whole blocks, one lane each, six chained E_K
        msgs = torch.randint(0, 256, (n * 6 * 16,), dtype=torch.uint8, device="cuda", generator=g)
        civ = torch.randint(0, 256, (n * 16,), dtype=torch.uint8, device="cuda", generator=g)
        sc = [window(lambda: eng.beltCBCEncr_batch_dev(msgs, 6, kw, civ), sync) for _ in range(3)]
        e["belt_cbc_encr_kernel"] = {"blocks_per_message": 6, "messages_per_s_runs": [n / s for s in sc], "messages_per_s": n / med(sc)}
        e["encr_over_cbc6"] = e["encr_records_per_s"] / e["belt_cbc_encr_kernel"]["messages_per_s"]
        out["shapes"].append(e)
        print(json.dumps(e), flush=True)
        del data, ivs, ct, pt, msgs, civ


def fold_part(out, parent_lib, mirrored=False):
    """bench.py --full with the parent's library and with this one, three times each, parent first in every pair; mirrored: this
    first"""
    runs = {"parent": [], "this": []}
    for rnd in range(3):
        for which in (("this", "parent") if mirrored else ("parent", "this")):
            env = dict(os.environ)
            if which == "parent":
                env["BEE2HIP_LIB"] = os.path.abspath(parent_lib)
            else:
                env.pop("BEE2HIP_LIB", None)
            t0 = time.perf_counter()
            run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--full", "--steps", "5", "--warmup", "2"],
                                 cwd=ROOT, env=env, check=True, timeout=500, stdout=subprocess.PIPE, text=True)
            line = json.loads(run.stdout.strip().splitlines()[-1])      # the bench's JSON line names its detail file (every leg's record)
            d = json.load(open(os.path.join(ROOT, line["detail"])))
            legs = {d["headline"]["metric"]: d["headline"]["value"]}
            legs.update({name: rec["value"] for name, rec in d["others"].items() if isinstance(rec, dict) and "value" in rec})
            runs[which].append(legs)
            print(which, f"{time.perf_counter() - t0:.0f} s", legs, flush=True)
    keys = sorted(runs["this"][0])
    spread = {k: [min(r[k] for r in runs["parent"]), max(r[k] for r in runs["parent"])] for k in keys}
    out["fold_non_regression_mirrored" if mirrored else "fold_non_regression"] = {
        "command": "bench.py --gpus 1 --full --steps 5 --warmup 2", "runs": runs, "parent_spread": spread,
        "this_inside_parent_spread": {k: [spread[k][0] <= r[k] <= spread[k][1] for r in runs["this"]] for k in keys}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "belt_fmt_rate.json"))
    ap.add_argument("--fold", metavar="PARENT_LIB", default=None, help="libbee2hip.so built from the parent commit")
    ap.add_argument("--mirrored", action="store_true", help="--fold with this library first in every pair")
    ap.add_argument("--skip-rates", action="store_true")
    args = ap.parse_args()
    out = {}
    if os.path.exists(args.out):
        out = json.load(open(args.out))
    if args.fold:                       # first: the bench runs in processes of their own, before this one opens the GPU
        fold_part(out, args.fold, args.mirrored)
    if not args.skip_rates:
        gpu_part(out, SHAPES)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
