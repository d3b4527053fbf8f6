"""Rates of the bash-prg batch entries on one GPU -> profiles/bashprg_rate.json (README "where it stands").

  1. prg-hash (l, d) = (128, 2) -- rate 128, bash256's -- against bee2hip_hash_ragged_dev(alg = 128) on the same 2^18 x 1000 B batch,
     alternating; the existing kernel is the yardstick, the ratio is recorded, no threshold
  2. prg-ae wrap and unwrap, (128, 2) and (256, 1), records of 64 B, 1000 B and 16 KiB: GiB/s and records/s, and the reference
     (oracle/_ref/libbee2ref.so) called from 16 threads on a sample of the same records
  3. one record of 256 KiB alone: the price of having no 8-lane form
  4. --fold PARENT_LIB: `bench.py --only ragged` with the parent's library and with this one, alternating, three times each; the
     *_caller_order figures (the path whose scan kernel was folded into the scatter)
Batches are device-resident and warmed up; a timed window is >= 0.5 s of back-to-back calls and ends in a synchronise."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


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
            return dt / reps, reps
        reps = max(2 * reps, int(reps * 1.2 * least / max(dt, 1e-6)) + 1)


def gpu_part(out):
    import numpy as np
    import torch
    import bee2_amd
    import refgen
    eng = bee2_amd.load()
    eng.set_device(0)
    sync = torch.cuda.synchronize
    out["device"] = torch.cuda.get_device_name(0)
    out["engine"] = eng.version()

    def batch(n, length, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        data = torch.randint(0, 256, (n * length + 16,), dtype=torch.uint8, device="cuda", generator=g)
        off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * length
        return data, off

    # 1. prg-hash against bash256
    n, length = 1 << 18, 1000
    data, off = batch(n, length, 1)
    dig = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    runs = {"bash256": [], "prg_hash_128_2": []}
    for _ in range(3):
        s, _r = window(lambda: eng.hash_ragged_dev(128, data, off, dig, n), sync)
        runs["bash256"].append(n * length / s / 2 ** 30)
        s, _r = window(lambda: eng.bashPrgHash_ragged_stream(128, 2, b"", data, off, dig, 32, n), sync)
        runs["prg_hash_128_2"].append(n * length / s / 2 ** 30)
    med = {k: sorted(v)[1] for k, v in runs.items()}
    out["hash_vs_bash256"] = {"batch": f"{n} x {length} B", "unit": "GiB/s", "runs": runs, "median": med,
                              "ratio_prg_over_bash256": med["prg_hash_128_2"] / med["bash256"]}
    print("hash", out["hash_vs_bash256"], flush=True)
    del data, off, dig

    # 2. prg-ae
    ref = ctypes.CDLL(refgen.REF_SO) if refgen.have_ref() else None
    if ref is not None:
        ref.bashPrg_keep.restype = ctypes.c_size_t
    out["ae"] = []
    key = bytes(range(32))
    for l, d in ((128, 2), (256, 1)):
        for length, n in ((64, 1 << 20), (1000, 1 << 18), (16384, 1 << 14)):
            data, off = batch(n, length, 2)
            anns = torch.randint(0, 256, (n * 16,), dtype=torch.uint8, device="cuda")
            ct = torch.empty_like(data)
            pt = torch.empty_like(data)
            tags = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
            codes = torch.ones(n, dtype=torch.int32, device="cuda")
            wrap = lambda: eng.bashPrgAE_ragged_stream(False, l, d, key, anns, 16, None, None, data, off, ct, tags, 8, n)
            unwrap = lambda: eng.bashPrgAE_ragged_stream(True, l, d, key, anns, 16, None, None, ct, off, pt, tags, 8, n, codes=codes)
            sw, _r = window(wrap, sync)
            su, _r = window(unwrap, sync)
            assert int(codes.abs().sum()) == 0 and torch.equal(pt[: n * length], data[: n * length])
            e = {"l": l, "d": d, "record_bytes": length, "records": n, "ann_len": 16, "tag_len": 8, "header": "empty",
                 "wrap_GiBps": n * length / sw / 2 ** 30, "wrap_records_per_s": n / sw,
                 "unwrap_GiBps": n * length / su / 2 ** 30, "unwrap_records_per_s": n / su}
            if ref is not None:
                from concurrent.futures import ThreadPoolExecutor
                sub = min(n, max(256, (8 << 20) // length))
                host = data[: sub * length].cpu().numpy().copy()
                ha = anns[: sub * 16].cpu().numpy().copy()
                htag = np.empty((sub, 8), dtype=np.uint8)
                keep = ref.bashPrg_keep()
                _sz = ctypes.c_size_t

                def work(r):
                    st = ctypes.create_string_buffer(keep)
                    for i in r:
                        ref.bashPrgStart(st, _sz(l), _sz(d), ctypes.c_void_p(ha.ctypes.data + 16 * i), _sz(16), key, _sz(32))
                        ref.bashPrgAbsorb(key, _sz(0), st)
                        ref.bashPrgEncr(ctypes.c_void_p(host.ctypes.data + length * i), _sz(length), st)
                        ref.bashPrgSqueeze(ctypes.c_void_p(htag[i].ctypes.data), _sz(8), st)
                t0 = time.perf_counter()
                with ThreadPoolExecutor(16) as ex:
                    list(ex.map(work, [range(t, sub, 16) for t in range(16)]))
                dt = time.perf_counter() - t0
                same = bool((ct[: sub * length].cpu().numpy() == host).all() and (tags[: sub * 8].cpu().numpy().reshape(sub, 8) == htag).all())
                e["cpu_reference"] = {"threads": 16, "sample_records": sub, "wrap_GiBps": sub * length / dt / 2 ** 30,
                                      "wrap_records_per_s": sub / dt, "outputs_equal": same,
                                      "note": "bashPrgStart / Absorb / Encr / Squeeze of the reference through ctypes from 16 Python "
                                              "threads: four foreign calls per record are in the figure"}
            out["ae"].append(e)
            print("ae", e, flush=True)
            del data, off, anns, ct, pt, tags, codes

    # 3. one long record alone
    length = 256 * 1024
    data, off = batch(1, length, 3)
    dst = torch.empty_like(data)
    tag = torch.empty(8, dtype=torch.uint8, device="cuda")
    ann = torch.zeros(16, dtype=torch.uint8, device="cuda")
    s, _r = window(lambda: eng.bashPrgAE_ragged_stream(False, 128, 2, key, ann, 16, None, None, data, off, dst, tag, 8, 1), sync)
    dig = torch.empty(32, dtype=torch.uint8, device="cuda")
    s8, _r = window(lambda: eng.hash_ragged_dev(128, data, off, dig, 1), sync)
    out["one_long_record"] = {"bytes": length, "l": 128, "d": 2, "wrap_ms": s * 1e3, "us_per_permutation": s / (length // 160 + 3) * 1e6,
                              "bash256_8_lane_form_ms": s8 * 1e3}
    print("long", out["one_long_record"], flush=True)


def fold_part(out, parent_lib):
    """bench.py --only ragged with the parent's library and with this one, alternating"""
    runs = {"parent": [], "this": []}
    for _ in range(3):
        for which in ("parent", "this"):
            env = dict(os.environ)
            if which == "parent":
                env["BEE2HIP_LIB"] = os.path.abspath(parent_lib)
            else:
                env.pop("BEE2HIP_LIB", None)
            run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--only", "ragged", "--full", "--no-cpu",
                                  "--steps", "5", "--warmup", "2"], cwd=ROOT, env=env, check=True, timeout=240, stdout=subprocess.PIPE, text=True)
            line = json.loads(run.stdout.strip().splitlines()[-1])      # the bench's JSON line names its detail file (every leg's record)
            d = json.load(open(os.path.join(ROOT, line["detail"])))["headline"]
            runs[which].append({k: d[k] for k in sorted(d) if k.endswith("_caller_order") or k.endswith("_uniform_1000B")})
            print(which, runs[which][-1], flush=True)
    keys = [k for k in runs["this"][0] if k.endswith("_caller_order")]
    spread = {k: [min(r[k] for r in runs["parent"]), max(r[k] for r in runs["parent"])] for k in keys}
    out["fold_non_regression"] = {"unit": "GiB/s", "runs": runs, "parent_spread": spread,
                                  "this_inside_parent_spread": {k: [spread[k][0] <= r[k] <= spread[k][1] for r in runs["this"]] for k in keys},
                                  "this_not_below_parent_min": {k: all(r[k] >= spread[k][0] for r in runs["this"]) for k in keys}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bashprg_rate.json"))
    ap.add_argument("--fold", metavar="PARENT_LIB", default=None, help="libbee2hip.so built from the parent commit")
    ap.add_argument("--skip-rates", action="store_true")
    args = ap.parse_args()
    out = {}
    if os.path.exists(args.out):
        out = json.load(open(args.out))
    if args.fold:                       # first: the bench runs in processes of their own, before this one opens the GPU
        fold_part(out, args.fold)
    if not args.skip_rates:
        gpu_part(out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
