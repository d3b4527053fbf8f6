"""Rates of the belt-dwp / belt-che record batch on one GPU -> profiles/belt_ae_ragged_rate.json.

  1. bee2hip_beltAE_ragged_stream, wrap and unwrap, both modes, on 2^20 x 64 B, 2^18 x 1000 B, 2^14 x 16 KiB and one record of
     256 KiB alone: GiB/s and records/s, windows of at least 0.5 s, wrap and unwrap alternating, three repeats each (median)
  2. beside each: the reference (oracle/_ref/libbee2ref.so: beltDWPWrap / beltCHEWrap) through ctypes from 16 threads on a
     sample of the same records, outputs compared -- a floor for bee2 -- and belt_cbc_encr_kernel
     (bee2hip_beltCBCEncr_batch_dev) on the same number of messages of the same number of blocks: one lane per message and one
     E_K per block without the multiplier, so the gap is what the per-lane GF(2^128) product costs
  3. --fold PARENT_LIB: `bench.py --only dwp` with the parent's library and with this one, alternating, three times each (the
     jump-ahead kernels of belt-bde and belt-che were folded into one)
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

SHAPES = ((64, 1 << 20), (1000, 1 << 18), (16384, 1 << 14), (256 * 1024, 1))
MODE_NAME = {0: "dwp", 1: "che"}


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
    for length, n in shapes:
        g = torch.Generator(device="cuda").manual_seed(length)
        data = torch.randint(0, 256, (n * length + 16,), dtype=torch.uint8, device="cuda", generator=g)
        off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * length
        ivs = torch.randint(0, 256, (n * 16,), dtype=torch.uint8, device="cuda", generator=g)
        ct, pt = torch.empty_like(data), torch.empty_like(data)
        tags = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
        codes = torch.ones(n, dtype=torch.int32, device="cuda")
        e = {"record_bytes": length, "records": n, "header": "empty", "modes": {}}
        for mode in (0, 1):
            wrap = lambda: eng.beltAE_ragged_stream(False, mode, key, ivs, None, None, data, off, ct, tags, n)
            unwrap = lambda: eng.beltAE_ragged_stream(True, mode, key, ivs, None, None, ct, off, pt, tags, n, codes=codes)
            sw, su = [], []
            for _ in range(3):
                sw.append(window(wrap, sync))
                su.append(window(unwrap, sync))
            assert int(codes.abs().sum()) == 0 and torch.equal(pt[: n * length], data[: n * length])
            m = {"wrap_GiBps_runs": [n * length / s / 2 ** 30 for s in sw], "unwrap_GiBps_runs": [n * length / s / 2 ** 30 for s in su],
                 "wrap_GiBps": n * length / med(sw) / 2 ** 30, "unwrap_GiBps": n * length / med(su) / 2 ** 30,
                 "wrap_records_per_s": n / med(sw), "unwrap_records_per_s": n / med(su), "wrap_ms": med(sw) * 1e3}
            if ref is not None:
                sub = min(n, max(16, (8 << 20) // length))
                src = data[: sub * length].cpu().numpy().copy()
                host = np.empty_like(src)
                hiv = ivs[: sub * 16].cpu().numpy().copy()
                htag = np.empty((sub, 8), dtype=np.uint8)
                f = getattr(ref, f"belt{MODE_NAME[mode].upper()}Wrap")

                def work(r):
                    for i in r:
                        f(ctypes.c_void_p(host.ctypes.data + length * i), ctypes.c_void_p(htag[i].ctypes.data),
                          ctypes.c_void_p(src.ctypes.data + length * i), _sz(length), None, _sz(0), key, _sz(32),
                          ctypes.c_void_p(hiv.ctypes.data + 16 * i))
                t0 = time.perf_counter()
                with ThreadPoolExecutor(16) as ex:
                    list(ex.map(work, [range(t, sub, 16) for t in range(16)]))
                dt = time.perf_counter() - t0
                same = bool((ct[: sub * length].cpu().numpy() == host).all() and (tags[: sub * 8].cpu().numpy().reshape(sub, 8) == htag).all())
                m["cpu_reference"] = {"threads": 16, "sample_records": sub, "wrap_GiBps": sub * length / dt / 2 ** 30,
                                      "wrap_records_per_s": sub / dt, "outputs_equal": same,
                                      "batch_over_reference": (n * length / med(sw)) / (sub * length / dt),
                                      "note": "one foreign call per record from 16 Python threads is in the figure: a floor for bee2"}
            e["modes"][MODE_NAME[mode]] = m
        # the like-for-like form without the multiplier: n messages of ceil(length / 16) whole blocks
        nblk = (length + 15) // 16
        msgs = torch.randint(0, 256, (n * nblk * 16,), dtype=torch.uint8, device="cuda", generator=g)
        civ = torch.randint(0, 256, (n * 16,), dtype=torch.uint8, device="cuda", generator=g)
        sc = [window(lambda: eng.beltCBCEncr_batch_dev(msgs, nblk, kw, civ), sync) for _ in range(3)]
        e["belt_cbc_encr_kernel"] = {"message_bytes": nblk * 16, "GiBps_runs": [n * nblk * 16 / s / 2 ** 30 for s in sc],
                                     "GiBps": n * nblk * 16 / med(sc) / 2 ** 30}
        for name, m in e["modes"].items():
            m["wrap_over_cbc"] = m["wrap_GiBps"] / e["belt_cbc_encr_kernel"]["GiBps"]
        out["shapes"].append(e)
        print(json.dumps(e), flush=True)
        del data, off, ivs, ct, pt, tags, codes, msgs, civ


def fold_part(out, parent_lib, mirrored=False):
    """bench.py --only dwp with the parent's library and with this one, alternating; mirrored: this / parent / parent / this / this /
    parent instead of parent first in every pair (does the place in the pair matter?), recorded beside the first set"""
    runs = {"parent": [], "this": []}
    for rnd in range(3):
        for which in (("this", "parent") if mirrored and rnd % 2 == 0 else ("parent", "this")):
            env = dict(os.environ)
            if which == "parent":
                env["BEE2HIP_LIB"] = os.path.abspath(parent_lib)
            else:
                env.pop("BEE2HIP_LIB", None)
            run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--only", "dwp", "--full", "--no-cpu",
                                  "--steps", "5", "--warmup", "2"], cwd=ROOT, env=env, check=True, timeout=300, stdout=subprocess.PIPE, text=True)
            line = json.loads(run.stdout.strip().splitlines()[-1])      # the bench's JSON line names its detail file (every leg's record)
            d = json.load(open(os.path.join(ROOT, line["detail"])))["headline"]      # --only dwp: the leg's record is the headline
            runs[which].append({"dwp_wrap": d["value"], "mac_only": d["mac_only"], "che_wrap": d["che_wrap"]})
            print(which, runs[which][-1], flush=True)
    keys = sorted(runs["this"][0])
    spread = {k: [min(r[k] for r in runs["parent"]), max(r[k] for r in runs["parent"])] for k in keys}
    out["fold_non_regression_mirrored" if mirrored else "fold_non_regression"] = {"unit": "GiB/s", "command": "bench.py --gpus 1 --only dwp --full --no-cpu --steps 5 --warmup 2", "runs": runs,
                                  "parent_spread": spread,
                                  "this_inside_parent_spread": {k: [spread[k][0] <= r[k] <= spread[k][1] for r in runs["this"]] for k in keys}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "belt_ae_ragged_rate.json"))
    ap.add_argument("--fold", metavar="PARENT_LIB", default=None, help="libbee2hip.so built from the parent commit")
    ap.add_argument("--mirrored", action="store_true", help="--fold in the order this / parent / parent / this / this / parent")
    ap.add_argument("--skip-rates", action="store_true")
    ap.add_argument("--quick", action="store_true", help="the 64 B and 1000 B shapes only, no host reference (A/B of kernel forms)")
    args = ap.parse_args()
    out = {}
    if os.path.exists(args.out):
        out = json.load(open(args.out))
    if args.fold:                       # first: the bench runs in processes of their own, before this one opens the GPU
        fold_part(out, args.fold, args.mirrored)
    if not args.skip_rates:
        gpu_part(out, SHAPES[:2] if args.quick else SHAPES, not args.quick)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
