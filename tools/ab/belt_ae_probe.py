"""A few belt-dwp / belt-che record batches of 2^16 x 1000 B and nothing else on the GPU, for a counter run of its own:
rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_INSTS_LDS SQ_INSTS_VALU SQ_WAVES --output-format csv -d <dir> -o b -- python tools/ab/belt_ae_probe.py [mode] [reps]
(profiles/belt_ae_ragged_rate.json "lds_counters")."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT]
import torch  # noqa: E402
import bee2_amd  # noqa: E402

mode = int(sys.argv[1]) if len(sys.argv) > 1 else 0
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
eng = bee2_amd.load()
eng.set_device(0)
n, length = 1 << 16, 1000
g = torch.Generator(device="cuda").manual_seed(7)
data = torch.randint(0, 256, (n * length + 16,), dtype=torch.uint8, device="cuda", generator=g)
ivs = torch.randint(0, 256, (n * 16,), dtype=torch.uint8, device="cuda", generator=g)
off = torch.arange(n + 1, dtype=torch.int64, device="cuda") * length
order = torch.arange(n, dtype=torch.int32, device="cuda")
ct = torch.empty_like(data)
tags = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
for _ in range(reps):
    eng.beltAE_ragged_stream(False, mode, bytes(range(32)), ivs, None, None, data, off, ct, tags, n, order=order)
torch.cuda.synchronize()
print("done", n, length, mode, reps)
