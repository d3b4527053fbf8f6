"""Step plans for the drop-in streams whose steps change engine from call to call (bee2_amd/csrc/staging.hpp, with_host()):
which Step* calls a stream makes, how long each is, and -- from a model of the entry points in capi_belt.hip / capi_bash.hip --
which helper calls each step makes, with what size, and what partial block it leaves pending.  Pure Python, no oracle and no GPU:
tests/test_stream_plans.py proves on the CPU that the plans hold what tests/test_gpu_stream_handover.py relies on, and the GPU
test ties the model (the thresholds below, the calls per step) to the library's path counters.

A plan is a list of ops (kind, length): kind is the letter of the Step function ("E", "D", "I", "A", "H") or "G" / "V" (a tag or
digest in mid-stream, length 0).  simulate() walks a plan and returns one Step per op."""
import random
from collections import namedtuple

# ---- who runs where in auto mode: host_wanted(), bee2_amd/csrc/staging.hpp:403-405 (K_SERIAL: the default branch, :408)
K_PRIM, K_PARALLEL, K_SERIAL, K_POLY = 0, 1, 2, 3
PRIM_HOST_MAX = 1024                # K_PRIM: host when bytes <= 1024
PARALLEL_GPU_MIN = 8192             # K_PARALLEL: host when bytes < 8192
POLY_HOST_MAX_CLMUL = 32768         # K_POLY: host when bytes <= 32768 with PCLMULQDQ on the host ...
POLY_HOST_MAX_TABLE = 4096          # ... <= 4096 without
BLOCK = 16
MAX_PLAN_BYTES = 256 * 1024

# the sizes at which a kind changes engine: a plan has a bulk call exactly there, one block below and one block above
THRESHOLDS = {K_PARALLEL: (PARALLEL_GPU_MIN,), K_POLY: (POLY_HOST_MAX_TABLE, POLY_HOST_MAX_CLMUL)}

PARALLEL_LENGTHS = (1, 15, 16, 17, 8176, 8191, 8192, 8193, 8208, 20000)
POLY_LENGTHS = (16, 4080, 4096, 4112, 32752, 32768, 32784, 70000)
SUB_BLOCK = (3, 5, 11, 13)          # leave reserved / filled non-zero before a large step and after one


def host_in_auto(kind, nbytes, clmul):
    """host_wanted() with no BEE2HIP_FORCE: True = the call stays on the calling core"""
    if kind == K_PRIM:
        return nbytes <= PRIM_HOST_MAX
    if kind == K_PARALLEL:
        return nbytes < PARALLEL_GPU_MIN
    if kind == K_POLY:
        return nbytes <= (POLY_HOST_MAX_CLMUL if clmul else POLY_HOST_MAX_TABLE)
    return True


# one op of a plan as the library serves it: calls = the with_host() calls in order, (kind, bytes) each; pending_* = octets of a
# partial block the state holds before / after the op -- for "E" / "D" the unused gamma (`reserved`), for "I" / "A" / "H" the
# buffered input (`filled`, the sponge's `pos`), 0 for the modes whose state has no such field
Step = namedtuple("Step", "op n pending_before pending_after calls")

FAMILIES = ("CTR", "ECB-E", "ECB-D", "CBC-E", "CBC-D", "BDE-E", "BDE-D", "DWP", "CHE", "MAC", "HASH",
            "BASH128", "BASH192", "BASH256", "BASH80")
# families whose bulk kind has a size crossover (the auto-mode tests); the others are K_SERIAL: always the host in auto mode
CROSSOVER_FAMILIES = ("CTR", "ECB-E", "ECB-D", "CBC-D", "BDE-E", "BDE-D", "DWP", "CHE")
# belt_ecb_st, belt_cbc_st and belt_bde_st keep no partial block between steps (capi_belt.hip:290-293,827-831,744-749: every step
# but a stream's last is whole blocks), and the belt-mac look-ahead block is never empty once data has come
NO_PENDING_FIELD = ("ECB-E", "ECB-D", "CBC-E", "CBC-D", "BDE-E", "BDE-D")
BASH_LEVEL = {"BASH128": 128, "BASH192": 192, "BASH256": 256, "BASH80": 80}


def bulk_kind(family, op):
    """the kind of the op's size-dependent call"""
    if family in ("DWP", "CHE"):
        return K_PARALLEL if op in "ED" else K_POLY
    if family in ("CTR", "ECB-E", "ECB-D", "CBC-D", "BDE-E", "BDE-D"):
        return K_PARALLEL
    return K_SERIAL


class _Model:
    """the bookkeeping of the Step functions, without the arithmetic"""

    def __init__(self, family):
        self.family = family
        self.reserved = 0           # CTR / DWP / CHE: gamma octets left
        self.filled = 0             # DWP / CHE / MAC / HASH: buffered octets; bash: pos
        self.crit = 0               # DWP / CHE: octets given to StepA so far
        self.rate = 192 - BASH_LEVEL[family] // 2 if family in BASH_LEVEL else 0

    def _feed(self, n, calls):      # dwp_feed(), capi_belt.hip:389-403
        if self.filled:
            take = min(16 - self.filled, n)
            self.filled += take
            n -= take
            if self.filled < 16:
                return
            calls.append((K_POLY, 16))
            self.filled = 0
        full = n & ~15
        if full:
            calls.append((K_POLY, full))
        self.filled = n - full

    def step(self, op, n):
        f, calls = self.family, []
        if op in "ED" and f in ("CTR", "DWP", "CHE"):
            before = self.reserved
            take = min(self.reserved, n)
            self.reserved -= take
            n -= take
            if f == "CHE":          # beltCHEStepE, capi_belt.hip:681-703
                if n // 16:
                    calls.append((K_PARALLEL, n // 16 * 16))
                if n % 16:
                    calls.append((K_PRIM, 16))
                    self.reserved = 16 - n % 16
            elif not (before and n == 0):      # ctr_bulk, capi_belt.hip:80-86,129: the whole rest in one call
                calls.append((K_PARALLEL, n))
                if n:
                    self.reserved = (16 - n % 16) % 16
            return Step(op, n + take, before, self.reserved, tuple(calls))
        if f in ("ECB-E", "ECB-D"):             # ecb_step, capi_belt.hip:300-314
            if n // 16:
                calls.append((K_PARALLEL, n // 16 * 16))
            if n % 16:
                calls.append((K_PRIM, 16))
        elif f == "CBC-E":                      # beltCBCStepE, capi_belt.hip:840-869
            if n // 16:
                calls.append((K_SERIAL, n // 16 * 16))
            if n % 16:
                calls.append((K_PRIM, 16))
        elif f == "CBC-D":                      # beltCBCStepD, capi_belt.hip:871-895
            par = n // 16 - 1 if n % 16 else n // 16
            if par:
                calls.append((K_PARALLEL, par * 16))
            if n % 16:
                calls += [(K_PRIM, 16), (K_PRIM, 16)]
        elif f in ("BDE-E", "BDE-D"):           # bde_host, capi_belt.hip:773-796
            if n // 16:
                calls.append((K_PARALLEL, n // 16 * 16))
        elif f in ("DWP", "CHE"):
            before = self.filled
            if op == "I":
                self._feed(n, calls)
            elif op == "A":                     # beltDWPStepA, capi_belt.hip:410-419: the open data is padded first
                if n and self.crit == 0 and self.filled:
                    calls.append((K_POLY, self.filled))
                    self.filled = 0
                self.crit += n
                self._feed(n, calls)
            else:                               # dwp_tag, capi_belt.hip:421-436: the state is not disturbed
                calls += [(K_POLY, 32 if self.filled else 16), (K_PRIM, 16)]
            return Step(op, n, before, self.filled, tuple(calls))
        elif f == "MAC":
            before = self.filled
            if op == "A":                       # beltMACStepA, capi_belt.hip:176-186
                if self.filled < 16 and n <= 16 - self.filled:
                    self.filled += n
                else:
                    calls.append((K_SERIAL, n))
                    self.filled = (self.filled + n - 1) % 16 + 1
            else:
                calls.append((K_SERIAL, 0))
            return Step(op, n, before % 16, self.filled % 16, tuple(calls))
        elif f == "HASH":
            before, n0 = self.filled, n
            if op == "H":                       # beltHashStepH, capi_belt.hip:503-522
                if self.filled:
                    take = min(32 - self.filled, n)
                    self.filled += take
                    n -= take
                    if self.filled < 32:
                        return Step(op, n0, before, self.filled, ())
                    calls.append((K_SERIAL, 32))
                    self.filled = 0
                if n // 32:
                    calls.append((K_SERIAL, n // 32 * 32))
                self.filled = n % 32
            else:                               # hash_digest, capi_belt.hip:523-532
                calls.append((K_SERIAL, 32 if self.filled else 0))
            return Step(op, n0, before, self.filled, tuple(calls))
        elif f in BASH_LEVEL:
            before = self.filled
            if op == "H":                       # bashHashStepH, capi_bash.hip:55-65
                if n < self.rate - self.filled:
                    self.filled += n
                else:
                    calls.append((K_SERIAL, n))
                    self.filled = (self.filled + n) % self.rate
            else:
                calls.append((K_PRIM, 192))
            return Step(op, n, before, self.filled, tuple(calls))
        return Step(op, n, 0, 0, tuple(calls))


def simulate(family, ops):
    m = _Model(family)
    return [m.step(op, n) for op, n in ops]


def bulk_call(family, step):
    """(kind, bytes) of the step's largest call of its size-dependent kind, or None when the step made none"""
    kind = bulk_kind(family, step.op)
    sizes = [b for k, b in step.calls if k == kind]
    return (kind, max(sizes)) if sizes else None


def is_large(family, step, clmul):
    """the step has a call that auto mode sends to the GPU (K_SERIAL families: a call of SERIAL_LARGE octets or more -- auto mode
    keeps them on the host, the forced patterns do not)"""
    b = bulk_call(family, step)
    if b is None:
        return False
    if b[0] == K_SERIAL:
        return b[1] >= SERIAL_LARGE
    return not host_in_auto(b[0], b[1], clmul)


def predicted_counts(step, clmul):
    """(host calls, GPU calls) of a step in auto mode"""
    host = sum(1 for k, b in step.calls if host_in_auto(k, b, clmul))
    return host, len(step.calls) - host


def total_bytes(ops):
    return sum(n for _, n in ops)


# ------------------------------------------------------------------ the plans ---
def _ops(op, lengths):
    return [(op, n) for n in lengths]


# gamma streams (CTR, the E / D side of DWP and CHE).  Aligned: bulk sizes exactly at, one block below and one block above 8192 from
# a block boundary.  Pending: large steps entered and left inside a gamma block -- 5 leaves reserved = 11, 8203 = 11 + 8192 is a bulk
# call exactly at the threshold, 8214 enters with 11 and leaves 5, 8191 after 14 left over is a bulk call of 8177 (host) ...
_GAMMA_ALIGNED = (16, 8176, 8192, 8208, 16, 8192, 8192, 1, 15, 17, 15, 8193, 8191)
_GAMMA_PENDING = (5, 8203, 8197, 8214, 7, 8191, 8207, 20000, 3, 8189, 13, 20000, 1, 8210, 15)
# whole-block streams (ECB, CBC, BDE): the stealing tail of ECB / CBC only in the last step
_BLOCKS = (16, 8176, 8192, 8208, 32, 8192, 20000, 16, 8192)
# polynomial streams (the I / A side of DWP and CHE): bulk sizes at, one block below and one block above both thresholds; then the
# same crossings with 5 octets buffered before the step and after it (4128 = 11 + 4112 + 5, 32800 = 11 + 32784 + 5)
_POLY_ALIGNED = (16, 4080, 4096, 4112, 16, 4112, 32752, 32768, 32784, 32784, 16, 70000)
_POLY_PENDING = (5, 4123, 21, 4128, 4128, 27, 21, 32800, 32800, 27, 3, 70000, 13)
# serial chains (MAC, belt-hash, bash, CBC encryption): no crossover; the sizes around a block, around the 2 KiB at which chain
# staging leaves the pinned buffer (staging.hpp:238), around the 4 KiB at which a bash step changes kernel (capi_bash.hip:39)
SERIAL_LARGE = 4096
_SERIAL = (1, 15, 16, 17, 31, 32, 33, 2047, 2049, 5, 4095, 4096, 4097, 11, 9000, 8192, 3, 20000, 127, 129, 4300, 6000, 7, 5000)


def _ae_plans():
    """belt-dwp / belt-che: I ..., then E and A in turn with a tag in mid-stream, V at the end; and the order of an unwrap: I, A, V, D"""
    out = {}
    for name, poly in (("poly-aligned", _POLY_ALIGNED), ("poly-pending", _POLY_PENDING)):
        ops = _ops("I", poly[:6]) + [("G", 0)]
        for k, a in enumerate(poly[6:]):
            ops += [("E", (16, 5, 27)[k % 3]), ("A", a)]
            if k == 2:
                ops.append(("G", 0))
        out[name] = ops + [("G", 0), ("V", 0)]
    for name, gamma in (("gamma-aligned", _GAMMA_ALIGNED), ("gamma-pending", _GAMMA_PENDING)):
        ops = [("I", 16), ("I", 7)]
        for k, e in enumerate(gamma):
            ops += [("E", e), ("A", (16, 5, 27, 48)[k % 4])]
            if k == 4:
                ops.append(("G", 0))
        out[name] = ops + [("G", 0), ("V", 0)]
    out["unwrap"] = [("I", 5), ("I", 4123), ("A", 7), ("A", 32793), ("A", 8213), ("G", 0), ("V", 0),
                     ("D", 7), ("D", 8213), ("D", 20000), ("D", 12573), ("D", 3)]
    return out


def plans(family):
    """name -> ops"""
    if family == "CTR":
        return {"aligned": _ops("E", _GAMMA_ALIGNED), "pending": _ops("E", _GAMMA_PENDING)}
    if family in NO_PENDING_FIELD:
        op = family[-1]
        out = {"blocks": _ops(op, _BLOCKS)}
        if family[:3] != "BDE":
            out["steal-small"] = _ops(op, (8192, 16, 8208, 23))
            out["steal-large"] = _ops(op, (16, 8192, 8176, 8215))
        return out
    if family in ("DWP", "CHE"):
        return _ae_plans()
    if family == "MAC" or family == "HASH" or family in BASH_LEVEL:
        op = "A" if family == "MAC" else "H"
        ops = []
        for k, n in enumerate(_SERIAL):
            ops.append((op, n))
            if k % 4 == 3:
                ops.append(("G", 0))
        end = [("G", 0), ("V", 0)] if family == "MAC" else [("G", 0)]
        # and large steps that start and end on a block boundary of the chain (MAC: the first 16 octets are only buffered)
        B = 16 if family == "MAC" else 32 if family == "HASH" else 192 - BASH_LEVEL[family] // 2
        L = (SERIAL_LARGE + B - 1) // B * B
        return {"serial": ops + end, "aligned": _ops(op, (B, L, L + B, B, L)) + end}
    raise KeyError(family)


def pattern(name, n, seed=0):
    """the engine of each of n steps: 'g' / 'c'"""
    if name == "gc":
        return "gc" * (n // 2) + "g" * (n % 2)
    if name == "cg":
        return "cg" * (n // 2) + "c" * (n % 2)
    rnd = random.Random(0x57E9 ^ seed)
    return "".join(rnd.choice("gc") for _ in range(n))


PATTERNS = ("gc", "cg", "random")


def orders(family, ops, clmul):
    """{(kind, class of the previous step, class of this step, partial block pending before this step)} over adjacent steps that both
    make a call of the size-dependent kind; class 'L' = is_large(), else 'S'.  For the AE families E / D steps (K_PARALLEL) and
    I / A steps (K_POLY) are two streams through one state: each is followed separately."""
    have = set()
    last = {}
    for st in simulate(family, ops):
        if st.op in "GV" or bulk_call(family, st) is None:
            continue
        lane = bulk_kind(family, st.op)
        cls = "L" if is_large(family, st, clmul) else "S"
        if lane in last:
            have.add((lane, last[lane], cls, st.pending_before != 0))
        last[lane] = cls
    return have


def bulk_sizes(family, ops):
    """{kind: sizes of every call of the size-dependent kinds over a plan}"""
    out = {}
    for st in simulate(family, ops):
        for k, b in st.calls:
            if k in (K_PARALLEL, K_POLY):
                out.setdefault(k, set()).add(b)
    return out
