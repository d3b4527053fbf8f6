"""TEST INFRASTRUCTURE: pure-Python restatement of bignVerify / bignPubkeyVal / bignPubkeyCalc / bignSign over an ARBITRARY parameter set
(bign_sign.c:268-361, bign_misc.c:319-365, bign_params.c:244-280, bign_ec.c:29-80), big integers and textbook affine
formulas; belt-hash comes from the C oracle (orclib).  Pinned by tests/test_oracle_golden.py against
tests/golden/bign_generic.json, which the reference itself produced (tools/make_golden_generic.py)."""

ERR_OK, ERR_BAD_INPUT, ERR_NOT_IMPLEMENTED = 0, 109, 119
ERR_BAD_PARAMS, ERR_BAD_PUBKEY, ERR_BAD_SIG = 502, 505, 510


def le(b):
    return int.from_bytes(bytes(b), "little")


class Params:
    def __init__(self, l, p, a, b, q, yG):
        self.l, self.p, self.a, self.b, self.q, self.yG = l, bytes(p), bytes(a), bytes(b), bytes(q), bytes(yG)

    @classmethod
    def from_hex(cls, d):
        return cls(d["l"], *(bytes.fromhex(d[k]) for k in ("p", "a", "b", "q", "yG")))


def params_check(P):
    """bignParamsCheck followed by what bignEcCreate rejects; the 64-octet fields arrive zero-padded"""
    l = P.l
    if 2 * l % 64:
        return ERR_NOT_IMPLEMENTED
    no = 2 * l // 8
    if no == 0 or no > 64:
        return ERR_BAD_PARAMS
    pad = lambda x: bytes(x) + bytes(64 - len(x))
    p, a, b, q, yG = (pad(x) for x in (P.p, P.a, P.b, P.q, P.yG))
    ok = (p[0] % 4 == 3 and q[0] % 2 == 1 and p[no - 1] >= 128 and q[no - 1] >= 128 and not any(p[no:])
          and any(a[:no]) and any(b[:no]) and not any(a[no:]) and not any(b[no:]) and not any(q[no:]) and not any(yG[no:]))
    if not ok:
        return ERR_BAD_PARAMS
    if l % 64:
        return ERR_NOT_IMPLEMENTED
    if l not in (128, 192, 256):
        return ERR_BAD_PARAMS
    pi = le(p[:no])
    if le(a[:no]) >= pi or le(b[:no]) >= pi or le(yG[:no]) >= pi:      # qrFrom in ecpCreateJ / ecGroupCreate
        return ERR_BAD_PARAMS
    return ERR_OK


def _add(P1, P2, a, p):
    if P1 is None:
        return P2
    if P2 is None:
        return P1
    x1, y1 = P1
    x2, y2 = P2
    if x1 == x2:
        if (y1 + y2) % p == 0:
            return None
        lam = (3 * x1 * x1 + a) * pow(2 * y1, -1, p) % p
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, p) % p
    x3 = (lam * lam - x1 - x2) % p
    return x3, (lam * (x1 - x3) - y1) % p


def mul(k, P, a, p):
    R = None
    for i in reversed(range(k.bit_length())):
        R = _add(R, R, a, p)
        if (k >> i) & 1:
            R = _add(R, P, a, p)
    return R


def verify(P, oid_der, h, sig, pub, belt_hash):
    code = params_check(P)
    if code:
        return code
    l = P.l
    no = l // 4
    p, a, q, yG = le(P.p[:no]), le(P.a[:no]), le(P.q[:no]), le(P.yG[:no])
    x, y = le(pub[:no]), le(pub[no:2 * no])
    if x >= p or y >= p:
        return ERR_BAD_PUBKEY
    s0, s1 = le(sig[:no // 2]), le(sig[no // 2:no // 2 + no])
    if s1 >= q:
        return ERR_BAD_SIG
    H = le(h[:no])
    if H >= q:
        H -= q
    u = (s1 + H) % q
    v = s0 + (1 << l)
    R = _add(mul(u, (0, yG), a, p), mul(v, (x, y), a, p), a, p)
    if R is None:
        return ERR_BAD_SIG
    t = belt_hash(bytes(oid_der) + R[0].to_bytes(no, "little") + bytes(h[:no]))
    return ERR_OK if t[:no // 2] == bytes(sig[:no // 2]) else ERR_BAD_SIG


def pubkey_val(P, pub):
    code = params_check(P)
    if code:
        return code
    no = P.l // 4
    p, a, b = le(P.p[:no]), le(P.a[:no]), le(P.b[:no])
    x, y = le(pub[:no]), le(pub[no:2 * no])
    if x >= p or y >= p:
        return ERR_BAD_PUBKEY
    return ERR_OK if (y * y - (x * x * x + a * x + b)) % p == 0 else ERR_BAD_PUBKEY


ERR_BAD_RNG, ERR_BAD_PRIVKEY = 304, 504


def pubkey_calc(P, priv):
    """bignPubkeyCalc (bign_misc.c:373-429): ERR_BAD_PRIVKEY unless 0 < d < q, then Q = d G by affine arithmetic
    (ERR_BAD_PARAMS if that is O).  Returns (code, pubkey)."""
    code = params_check(P)
    if code:
        return code, b""
    no = P.l // 4
    p, a, q, yG = le(P.p[:no]), le(P.a[:no]), le(P.q[:no]), le(P.yG[:no])
    d = le(priv[:no])
    if d == 0 or d >= q:
        return ERR_BAD_PRIVKEY, b""
    Q = mul(d, (0, yG), a, p)
    if Q is None:
        return ERR_BAD_PARAMS, b""
    return ERR_OK, Q[0].to_bytes(no, "little") + Q[1].to_bytes(no, "little")


def sign_k(P, oid_der, h, priv, k, belt_hash):
    """bignSign once its generator has produced the one-time key k (bign_sign.c:76-115): ERR_BAD_PRIVKEY unless 0 < d < q,
    ERR_BAD_RNG unless 0 < k < q (zzRandNZMod accepts exactly that range), R = k G, s0 = belt-hash(oid || x_R || H) cut to
    l bits, s1 = (k - (s0 + 2^l) d - H) mod q with H reduced by one subtraction.  Returns (code, sig)."""
    code = params_check(P)
    if code:
        return code, b""
    l = P.l
    no = l // 4
    p, a, q, yG = le(P.p[:no]), le(P.a[:no]), le(P.q[:no]), le(P.yG[:no])
    d, kk = le(priv[:no]), le(k[:no])
    if d == 0 or d >= q:
        return ERR_BAD_PRIVKEY, b""
    if kk == 0 or kk >= q:
        return ERR_BAD_RNG, b""
    R = mul(kk, (0, yG), a, p)
    if R is None:
        return ERR_BAD_PARAMS, b""
    s0 = belt_hash(bytes(oid_der) + R[0].to_bytes(no, "little") + bytes(h[:no]))[:no // 2]
    H = le(h[:no])
    if H >= q:
        H -= q
    s1 = (kk - (le(s0) + (1 << l)) * d - H) % q
    return ERR_OK, s0 + s1.to_bytes(no, "little")


def ladder_events(P, h, sig, pub):
    """The verification kernel's simultaneous double-and-add (bign_generic_verify_kernel: for i = 2l - 1 .. 0: T <- 2 T;
    T <- T + G if bit i of u; T <- T + Q if i <= l and bit i of v) replayed on affine points, recording which exceptional
    branch of the kernel's point arithmetic each step takes: "dbl Y == 0" (gj_dbl on a point of order 2), "add T == E"
    (gj_add falls into the doubling), "add T == -E" (gj_add returns O), "R == O" (the result), each with the bit index i of the step (-1
    for the result), in order.  Additions into or of O and doublings of O are ordinary early returns and are not recorded."""
    l = P.l
    no = l // 4
    p, a, q, yG = le(P.p[:no]), le(P.a[:no]), le(P.q[:no]), le(P.yG[:no])
    Q = (le(pub[:no]), le(pub[no:2 * no]))
    s0, s1 = le(sig[:no // 2]), le(sig[no // 2:no // 2 + no])
    H = le(h[:no])
    if H >= q:
        H -= q
    u, v = (s1 + H) % q, s0 + (1 << l)
    ev = []

    def add(T, E, i):
        if T is not None and E is not None and T[0] == E[0]:
            ev.append(("add T == E" if T[1] == E[1] and T[1] else "add T == -E", i))
        return _add(T, E, a, p)
    T = None
    for i in reversed(range(2 * l)):
        if T is not None and T[1] == 0:
            ev.append(("dbl Y == 0", i))
        T = _add(T, T, a, p)
        if (u >> i) & 1:
            T = add(T, (0, yG), i)
        if i <= l and (v >> i) & 1:
            T = add(T, Q, i)
    if T is None:
        ev.append(("R == O", -1))
    return ev
