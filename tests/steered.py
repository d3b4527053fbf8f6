"""tests/golden/bign_steered.json (tools/make_golden_steered.py): valid signatures whose verification scalars u = (s1 + H) mod q
and v = s0 + 2^l are STEERED -- zero comb windows of u, u = 0 / 1 / q - 1, empty windows of v under a shared key, accumulators that
meet the comb point they are about to add -- and their invalid neighbours.  A plain module: the reader, the windows of the scalars as
the kernels of bee2_amd/csrc/bign_kernels.hip cut them, and a Python-integer model of their walk.

The walk (bign_main_kernel, bign_main29_kernel, bign_onekey_kernel): T = v Q first, then the 16-bit comb windows of u in ASCENDING
order, T += u_j 2^(16 j) G for every non-zero u_j.  With Q = d G every point is a multiple of G, so the model keeps T as a number
mod q and names the steps at which the addition is exceptional: T == E (a doubling), T == -E (the sum is O), T == O."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "bign_steered.json")
LEVELS = (128, 192, 256)
FAMILIES = ("a", "b", "c", "d", "e")
ERR_BAD_SIG = 510


def nw(l):
    """16-bit comb windows of u: 2N for N 32-bit limbs"""
    return l // 8


def le(b):
    return int.from_bytes(bytes(b), "little")


class Steered:
    """the fixture, flattened: .q[l]; .cases = records with l, family, name, hash, sig, pubkey, code, U (+ key_index for c and d,
    d for d, parent and window for e); .signers[l] = [{"pubkey", "d" or None, "pool": [(hash, sig), ...]}, ...].  Octet strings
    are bytes, U / d / q are integers.  A record of family e is stored with its signature only: hash and key are its parent's."""

    def __init__(self, path=PATH):
        with open(path) as f:
            raw = json.load(f)
        self.q = {int(l): int(x, 16) for l, x in raw["q"].items()}
        self.cases, self.signers = [], {}
        for l in LEVELS:
            cur = raw["curves"][str(l)]
            by_name = {}
            for r in cur["cases"]:
                c = dict(r, l=l)
                if "parent" in c:
                    c["hash"], c["pubkey"] = by_name[c["parent"]]["hash"], by_name[c["parent"]]["pubkey"]
                else:
                    c["hash"], c["pubkey"] = bytes.fromhex(c["hash"]), bytes.fromhex(c["pubkey"])
                c["sig"] = bytes.fromhex(c["sig"])
                c["U"] = int(c["U"], 16)
                if "d" in c:
                    c["d"] = int(c["d"], 16)
                assert c["name"] not in by_name
                by_name[c["name"]] = c
                self.cases.append(c)
            self.signers[l] = [{"pubkey": bytes.fromhex(s["pubkey"]), "d": int(s["d"], 16) if "d" in s else None,
                                "pool": [(bytes.fromhex(h), bytes.fromhex(g)) for h, g in s["pool"]]} for s in cur["signers"]]

    def of(self, l, family=None):
        return [c for c in self.cases if c["l"] == l and (family is None or c["family"] == family)]


_cached = None


def load():
    global _cached
    if _cached is None:
        _cached = Steered()
    return _cached


# ---- the scalars of a signature, as bignVerify (bign_sign.c:320-327) and prep_scalars derive them
def u_of(l, q, hash_, sig):
    no = l // 4
    H = le(hash_)
    if H >= q:
        H -= q
    return (le(sig[no // 2:]) + H) % q


def v_of(l, sig):
    return le(sig[:l // 8]) + (1 << l)


def windows16(x, l):
    """the comb windows of u, window 0 first"""
    return [(x >> (16 * j)) & 0xFFFF for j in range(nw(l))]


def from_windows16(ws):
    return sum(w << (16 * j) for j, w in enumerate(ws))


def v_digits(v, l):
    """the l / 4 + 1 signed radix-16 digits of v, digit 0 first: nibble_i(v + 0x88...8) - 8, each in [-8, 7], the top one 1 or 2
    (prep_scalars; bign_main_kernel walks them from the top)"""
    n = l // 4 + 1
    w = v + sum(8 << (4 * i) for i in range(n))
    d = [((w >> (4 * i)) & 15) - 8 for i in range(n)]
    assert sum(x << (4 * i) for i, x in enumerate(d)) == v and d[-1] in (1, 2)
    return d


def s0_windows8(l, sig):
    """the windows of v below the top one on a key's 8-bit table: the octets of s0"""
    return list(sig[:l // 8])


def s0_windows16(l, sig):
    """... on its 16-bit table: the 16-bit words of s0"""
    return [sig[2 * i] | sig[2 * i + 1] << 8 for i in range(l // 16)]


# ---- the model
def walk(l, q, U, v, d):
    """-> [(step, kind)] of the exceptional additions of the serial walk: step = the comb window of u, kind = "E" (T == E), "-E"
    (T == -E) or "O" (T == O before the addition).  T starts as v d (v Q, Q = d G), window j adds u_j 2^(16 j)."""
    T = v * d % q
    out = []
    for j, w in enumerate(windows16(U, l)):
        if w == 0:
            continue                                   # the kernels skip the window: entry 0 of the comb is not a point
        E = (w << (16 * j)) % q
        if T == 0:
            out.append((j, "O"))
        elif T == E:
            out.append((j, "E"))
        elif (T + E) % q == 0:
            out.append((j, "-E"))
        T = (T + E) % q
    return out


def fold(q, U, v, d):
    """the last addition of the forms that sum u G apart from v Q (the helper quad): "E" when v Q == u G, "-E" when the sum is O,
    "O" when one side is empty, else None"""
    a, b = v * d % q, U % q
    if a == 0 or b == 0:
        return "O"
    return "E" if a == b else "-E" if (a + b) % q == 0 else None
