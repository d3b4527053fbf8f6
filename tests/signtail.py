"""tests/golden/bign_sign_tail.json (tools/make_golden_sign_tail.py): signatures on the three standard curves whose private key is
STEERED so that the tail of signing, s1 = (k - (s0 + 2^l) d - H) mod q, takes the branches no random draw reaches.  A plain module:
the reader and, with Python integers only, the tail as bign_sign_tail_kernel computes it (bee2_amd/csrc/bign_sign_kernels.hip:
mod_q_ct on the (N/2 + 1) x N-limb product, then sub_mod_q_ct twice; the host's sign<N> of host_bign_ct.hpp and oracle/bign_oracle.c
have to give the same octets).

The steering: s0 = belt-hash(oid || x(k G) || H) does not depend on d.  With k, H and the OID fixed s0 is read off a signature made
under any key; for a wanted residue r the key d = r / (s0 + 2^l) mod q makes (s0 + 2^l) d = r (mod q) exactly.

Names, with W = 2^(2l), cq = W - q, N = l / 16 limbs of 32 bits:
  r   = (s0 + 2^l) d mod q        what mod_q_ct returns
  u   = (k - r) mod q             the first sub_mod_q_ct
  s1  = u - H (+ q on a borrow)   the second one, zzSubMod with the RAW H: a residue unless H >= q and u < H - q (kind "wrap")
An EVENT of the fold is (top, t2, sub): the limb v[N] after the first fold v = lo + hi cq, the limb v[N] the second of the two
small passes meets, and whether the final masked subtraction of q is taken."""
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "bign_sign_tail.json")
LEVELS = (128, 192, 256)
KINDS = ("fold", "sub1", "sub2", "hge", "wrap")
ERR_BAD_SIG = 510


def le(b):
    return int.from_bytes(bytes(b), "little")


def curve_q(l):
    """q of the standard curve of level l, from the constants the product compiles (bee2_amd/csrc/bign_curves.inc)"""
    src = open(os.path.join(ROOT, "bee2_amd", "csrc", "bign_curves.inc")).read()
    m = re.search(r"k_bign%d_q\[[^\]]*\]\s*=\s*\{([^}]*)\}" % l, src)
    return le(bytes(int(x, 16) for x in re.findall(r"0x([0-9A-Fa-f]{2})", m.group(1))))


# ---- the fixture
class SignTail:
    """.records: dicts with l, kind, name and, as bytes, oid, priv, k, hash, sig, pub; verify = the reference's bignVerify code"""

    def __init__(self, path=PATH):
        with open(path) as f:
            raw = json.load(f)
        self.records = []
        for r in raw["records"]:
            c = dict(r)
            for f_ in ("oid", "priv", "k", "hash", "sig", "pub"):
                c[f_] = bytes.fromhex(c[f_])
            self.records.append(c)

    def of(self, l, kind=None):
        return [c for c in self.records if c["l"] == l and (kind is None or c["kind"] == kind)]


_cached = None


def load():
    global _cached
    if _cached is None:
        _cached = SignTail()
    return _cached


# ---- the tail in integers
def product(l, s0, d):
    """(s0 + 2^l) d: at most 3l + 1 bits, N + N/2 + 1 limbs"""
    return (s0 + (1 << l)) * d


def fold_passes(l, q, v):
    """what follows the first fold in mod_q_ct, on its value v = lo + hi cq -> ((top, t2, sub), v mod q)"""
    W = 1 << (2 * l)
    cq = W - q
    want = v % q
    assert v >> (2 * l + 32) == 0, "the first fold reaches limb N + 1, which the passes never read"
    top = v >> (2 * l)
    v = (v % W) + top * cq                               # pass 0, on N + 1 limbs
    assert v >> (2 * l + 32) == 0
    t2 = v >> (2 * l)
    v = (v % W) + t2 * cq                                # pass 1
    assert v >> (2 * l) == 0, "something is left above limb N - 1 after the two passes"
    sub = v >= q
    if sub:
        v -= q
    assert v == want
    return (top, t2, int(sub)), v


def fold_events(l, q, prod):
    """mod_q_ct<N, N + N/2 + 1> on prod -> ((top, t2, sub), prod mod q)"""
    W = 1 << (2 * l)
    assert 0 <= prod < 1 << (3 * l + 32)                 # N + N/2 + 1 limbs
    event, r = fold_passes(l, q, (prod % W) + (prod >> (2 * l)) * (W - q))          # v = lo + hi cq on N + 2 limbs
    assert r == prod % q
    return event, r


def sub_mod_q(l, q, a, b):
    """sub_mod_q_ct / zzSubMod: a - b on 2l bits, + q when that borrowed -> (the 2l-bit result, borrow).  b need not be below q."""
    W = 1 << (2 * l)
    borrow = int(a < b)
    return ((a - b) % W + (q if borrow else 0)) % W, borrow


def tail(l, q, s0, d, k, H):
    """-> dict(r, u, s1, event, borrow1, borrow2): the whole tail on integers; s1 as the 2l-bit number the signature carries"""
    event, r = fold_events(l, q, product(l, s0, d))
    u, b1 = sub_mod_q(l, q, k, r)
    s1, b2 = sub_mod_q(l, q, u, H)
    return {"r": r, "u": u, "s1": s1, "event": event, "borrow1": b1, "borrow2": b2}


def fold_bound(l, q):
    """-> (hi_max, v_max, m_max): d <= q - 1 and s0 + 2^l <= 2^(l+1) - 1 bound the high part of the product, hi <= hi_max =
    floor((2^(l+1) - 1)(q - 1) / W); then the first fold is at most v_max = (W - 1) + hi_max cq, and it is r + m q with
    m <= m_max = floor(v_max / q)."""
    W = 1 << (2 * l)
    hi_max = ((1 << (l + 1)) - 1) * (q - 1) // W
    v_max = (W - 1) + hi_max * (W - q)
    return hi_max, v_max, v_max // q


def all_events():
    """every (top, t2, sub) the three limbs could spell: top below 8 (the kernel's own comment), t2 and sub bits"""
    return [(top, t2, sub) for top in range(8) for t2 in (0, 1) for sub in (0, 1)]


def event_range(l, q, event):
    """-> (r_lo, r_hi), the residues r at which the bound of fold_bound lets the event happen, or a string saying why it cannot.

    Each pass and the final subtraction take a multiple of q off, so the first fold is v = r + m q with m = top + t2 + sub, and
    v = m W + (r - m cq) with 0 < r < q (r = 0 needs q | (s0 + 2^l) d, impossible for a prime q and factors below it: v == q never
    meets the final comparison).  m cq < W for every m <= m_max, hence
      r >= m cq            top = m,      pass 0 leaves r:              t2 = 0, sub = 0
      cq <= r < m cq       top = m - 1,  pass 0 leaves r + q >= W:     t2 = 1, sub = 0     (m >= 2)
      r < min(cq, m cq)    top = m - 1,  pass 0 leaves r + q < W:      t2 = 0, sub = 1     (m >= 1)"""
    W = 1 << (2 * l)
    cq = W - q
    _, v_max, m_max = fold_bound(l, q)
    assert (m_max + 1) * cq < W and v_max >> (2 * l + 32) == 0
    top, t2, sub = event
    m = top + t2 + sub
    if m > m_max:
        return "the first fold stays below %d q" % (m_max + 1)
    if t2 and sub:
        return "the top limb is m or m - 1: one more q at the most is left after pass 0"
    lo, hi = (m * cq, q - 1) if not (t2 or sub) else (cq, m * cq - 1) if t2 else (1, cq - 1)
    lo, hi = max(lo, 1), min(hi, q - 1, v_max - m * q)
    return (lo, hi) if lo <= hi else "no residue: [%#x, %#x] is empty" % (lo, hi)


def reachable(l, q):
    """-> {event: (r_lo, r_hi)}: every event the bound leaves possible"""
    out = {e: event_range(l, q, e) for e in all_events()}
    return {e: x for e, x in out.items() if not isinstance(x, str)}


def record_tail(c, q):
    """the tail of a fixture record, s0 taken from its signature"""
    l = c["l"]
    return tail(l, q, le(c["sig"][:l // 8]), le(c["priv"]), le(c["k"]), le(c["hash"]))


# ---- the plans of the kinds that need no search: (name, k, H, r) with r the residue the private key is to be solved for
def k_for(q, rnd, u, lo=1, hi=None):
    """a one-time key in [lo, hi] whose r = k - u is not 0"""
    hi = q - 1 if hi is None else hi
    while True:
        k = rnd.randrange(lo, hi + 1)
        if (k - u) % q:
            return k


def plan_sub1(l, q, rnd):
    k0, k1, k2 = rnd.randrange(1, q), rnd.randrange(1, q - 1), rnd.randrange(2, q)
    cases = [("u=0", k0, k0), ("u=q-1", k1, k1 + 1), ("u=1", k2, k2 - 1), ("k=1 r=q-1", 1, q - 1), ("k=q-1 r=1", q - 1, 1)]
    return [(name, k, rnd.randrange(q), r) for name, k, r in cases]


def plan_sub2(l, q, rnd):
    out = []
    for name in ("s1=0", "s1=q-1", "s1=1", "H=0", "H=q-1 u=0"):
        u = 0 if name == "H=q-1 u=0" else rnd.randrange(1, q - 1)
        k = k_for(q, rnd, u)
        H = {"s1=0": u, "s1=q-1": u + 1, "s1=1": u - 1, "H=0": 0, "H=q-1 u=0": q - 1}[name]
        out.append((name, k, H, (k - u) % q))
    return out


def _plan_hu(q, rnd, cases):
    out = []
    for name, H, u in cases:
        k = k_for(q, rnd, u)
        out.append((name, k, H, (k - u) % q))
    return out


def plan_hge(l, q, rnd):
    W = 1 << (2 * l)
    cq = W - q
    c = rnd.randrange(1, cq - 1)
    return _plan_hu(q, rnd, (("H=q u=0", q, 0), ("H=q+c u=c", q + c, c), ("H=q+c u=c+1", q + c, c + 1), ("H=W-1 u=cq-1", W - 1, cq - 1),
                             ("H=W-1 u=cq", W - 1, cq)))


def plan_wrap(l, q, rnd):
    W = 1 << (2 * l)
    cq = W - q
    return _plan_hu(q, rnd, (("H=W-1 u=0", W - 1, 0), ("H=W-1 u=cq-2", W - 1, cq - 2), ("H=q+1 u=0", q + 1, 0)))
