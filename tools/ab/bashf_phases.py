#!/usr/bin/env python3
"""python tools/ab/bashf_phases.py [--n STATES] [--stride S] [--launches L]   (on the GPU box)

Where a wavefront of bashF_tile_kernel spends its life.  Launches the stamped twin of the tile body (tools/probe/bashf_phases.hip,
bee2_amd/lib/libb2hphases.so) in both forms -- general = per-piece bounds on every tile, the kernel before the full-tile fast
path; fast = the product's body -- and prints, per cohort of resident workgroups (first / middle / last, by workgroup index:
a chip holds 6 workgroups per CU at a time), the median shader cycles and the median share of the wavefront's life of
  issue     entry -> loads issued            load wait   loads issued -> loaded data there
  rounds    the 24 rounds                    store 0/1   the two half-slab passes (fill, six reads, six stores issued)
The stamped build is slower than the product (stamps cost about 11 % of wave cycles and fence the scheduler): the SHARES are the
result, never its run time.  One stamp costs about 40 cycles; a phase of that size is noise."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIB = os.path.join(ROOT, "bee2_amd", "lib", "libb2hphases.so")
PHASES = [("issue", 0, 1), ("load wait", 1, 2), ("rounds", 2, 3), ("store 0", 3, 4), ("store 1", 4, 5)]


def stamps_of(lib, states, n, fast, stride, launches):
    grid = (n + 255) // 256
    cap = 8 * ((grid + stride - 1) // stride)
    buf = torch.zeros(cap, dtype=torch.int64, device="cuda")
    for _ in range(launches):                  # the last launch's stamps stay: the clock has settled by then
        rc = lib.b2h_bashf_phases(ctypes.c_void_p(states.data_ptr()), ctypes.c_size_t(n), int(fast), ctypes.c_void_p(buf.data_ptr()),
                                  ctypes.c_size_t(cap), ctypes.c_uint(stride), None)
        if rc != 0:
            raise RuntimeError(f"b2h_bashf_phases: {rc}")
    torch.cuda.synchronize()
    rows = buf.cpu().view(-1, 8).tolist()
    return [r for r in rows if r[5] > r[0] > 0]


def report(name, rows, grid, resident):
    print(f"== {name}: {len(rows)} stamped wavefronts, {grid} workgroups, {resident} resident at a time")
    cohorts = [("first", lambda w: w < resident), ("middle", lambda w: resident <= w < grid - resident),
               ("last", lambda w: w >= max(resident, grid - resident))]
    for cname, pick in cohorts:
        sel = [r for r in rows if pick(r[6])]
        if not sel:
            print(f"  {cname:6s} (no workgroup)")
            continue
        life = statistics.median(r[5] - r[0] for r in sel)
        line = f"  {cname:6s} n={len(sel):5d} life {life:7.0f} cyc |"
        edge = statistics.median(1 - (r[3] - r[2]) / (r[5] - r[0]) for r in sel)
        for pname, a, b in PHASES:
            cyc = statistics.median(r[b] - r[a] for r in sel)
            share = statistics.median((r[b] - r[a]) / (r[5] - r[0]) for r in sel)
            line += f" {pname} {cyc:6.0f} {100 * share:5.1f}% |"
        print(line + f" outside the rounds {100 * edge:5.1f}%")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--stride", type=int, default=4, help="every stride-th workgroup stamps (its wavefront 0)")
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args()
    if not os.path.exists(LIB):
        sys.exit(f"{LIB} is not built: python __graft_entry__.py")
    lib = ctypes.CDLL(LIB)
    lib.b2h_bashf_phases.restype = ctypes.c_int
    states = torch.randint(0, 256, (192 * a.n,), dtype=torch.uint8, device="cuda")
    grid = (a.n + 255) // 256
    resident = 6 * torch.cuda.get_device_properties(0).multi_processor_count
    print(f"bashF phases: {a.n} states, stride {a.stride}, stamps of launch {a.launches} of {a.launches}, {torch.cuda.get_device_name(0)}")
    for name, fast in (("general path on every tile (the kernel before the fast path)", 0), ("full-tile fast path (product body)", 1)):
        report(name, stamps_of(lib, states, a.n, fast, a.stride, a.launches), grid, resident)


if __name__ == "__main__":
    main()
