#!/usr/bin/env python3
"""python tools/ab/bashf_tile_ab.py --a <parent libbee2hip.so> --b <new libbee2hip.so> [--rounds 4] [--launches 60]   (on the GPU box)

A/B of two builds of libbee2hip.so on bashF_batch_dev, in the manner of tools/ab/ab_lib.sh: alternating rounds A, B, A, B ...
inside ONE job (boxes differ by several per cent), each round a fresh process under its own time limit that, after `warm` seconds of launches, times
`groups` groups of `launches` back-to-back launches, one event pair around each group as bench.py does (an event between every two
launches opens a gap of some 25 us behind each: 122 us per launch where bench.py reads 97), and prints the median of the
groups' per-launch times.  Sizes 2^20 (the headline) and 2^22 states.
The noise floor is the spread (max - min) of A's own round medians in this run; B passes at 2^20 when its median of round
medians is lower than A's by at least three times that spread, and at 2^22 when it is not worse by more than the spread there.
The last round of each size also reads the shader clock under the kernel (tools/probe/clock_probe.hip).
A round that fails or runs into its time limit ends the job: nothing more is started."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def worker(a):
    sys.path.insert(0, ROOT)
    import torch

    import bee2_amd
    eng = bee2_amd.load(a.lib)
    eng.set_device(0)
    st = torch.randint(0, 256, (192 * a.n,), dtype=torch.uint8, device="cuda")
    step = lambda: eng.bashF_batch_dev(st)  # noqa: E731
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < a.warm:                              # the clock settles under the kernel's own load
        for _ in range(100):
            step()
        torch.cuda.synchronize()
    us = []
    for _ in range(a.groups):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            step()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / a.launches)
    out = {"median_us": statistics.median(us), "mean_us": statistics.mean(us), "min_us": min(us)}
    if a.clock:
        from bench_legs.common import shader_clock_under
        out["ghz_under"], out["ghz_idle"] = shader_clock_under(step, out["median_us"] * 1e-3)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a"); ap.add_argument("--b")
    ap.add_argument("--rounds", type=int, default=4); ap.add_argument("--launches", type=int, default=60)
    ap.add_argument("--groups", type=int, default=50)
    ap.add_argument("--warm", type=float, default=0.5, help="seconds of back-to-back launches before the timed groups")
    ap.add_argument("--limit", type=int, default=120, help="seconds per round")
    ap.add_argument("--worker", action="store_true"); ap.add_argument("--lib"); ap.add_argument("--n", type=int); ap.add_argument("--clock", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    verdict = {}
    for n in (1 << 20, 1 << 22):
        med = {"A": [], "B": []}
        clock = {}
        for r in range(a.rounds):
            for tag, lib in (("A", a.a), ("B", a.b)):
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--lib", os.path.abspath(lib), "--n", str(n),
                       "--launches", str(a.launches), "--groups", str(a.groups), "--warm", str(a.warm)] + (["--clock"] if r == a.rounds - 1 else [])
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)      # the limit kills the round
                if p.returncode != 0:
                    sys.exit(f"round {r} {tag} n={n}: exit {p.returncode}\n{p.stderr[-2000:]}")
                d = json.loads(p.stdout.strip().splitlines()[-1])
                med[tag].append(d["median_us"])
                if "ghz_under" in d:
                    clock[tag] = d["ghz_under"]
                print(f"n=2^{n.bit_length() - 1} round {r} {tag}: median {d['median_us']:.2f} us  mean {d['mean_us']:.2f}  min {d['min_us']:.2f}"
                      + (f"  clock under the kernel {d['ghz_under']:.3f} GHz" if d.get("ghz_under") else ""), flush=True)
        A, B = statistics.median(med["A"]), statistics.median(med["B"])
        spread = max(med["A"]) - min(med["A"])
        print(f"n=2^{n.bit_length() - 1}: A {A:.2f} us (rounds {min(med['A']):.2f} .. {max(med['A']):.2f}, spread {spread:.2f})  "
              f"B {B:.2f} us (rounds {min(med['B']):.2f} .. {max(med['B']):.2f})  A - B = {A - B:.2f} us = {100 * (A - B) / A:.2f} %  "
              f"= {(A - B) / spread if spread else float('inf'):.1f} spreads  clocks A {clock.get('A')} B {clock.get('B')}", flush=True)
        verdict[n] = (A - B, spread)
    d20, s20 = verdict[1 << 20]
    d22, s22 = verdict[1 << 22]
    print(f"criterion 2^20: gain {d20:.2f} us >= 3 x spread {s20:.2f} us: {'MET' if d20 >= 3 * s20 else 'NOT MET'}")
    print(f"criterion 2^22: not worse by more than the spread {s22:.2f} us (gain {d22:.2f} us): {'MET' if d22 >= -s22 else 'NOT MET'}")


if __name__ == "__main__":
    main()
