"""The field and point arithmetic of the general-curve kernels (bee2_amd/csrc/bign_generic_kernels.hip: Montgomery CIOS on
32-bit limbs, g_mul / g_add / g_sub / g_inv, Jacobian gj_dbl / gj_add, the complete projective gp_add_complete, and the host
code that derives n0, R and R^2) against Python integers, bit-exact, through bee2hip_debug_feG of libbee2hip_exp.so -- on the
adversarial moduli of tests/golden/bign_generic_adv.json (tools/make_golden_generic_adv.py).

Random operands do not reach the rare words of the CIOS loop, so coverage is a CONDITION here: a word-level model of the
loop (cios_model, checked against a b R^-1 mod m on every call) counts four events per modulus,
    "spill"  t[N + 1] != 0 after the multiplication row of some iteration,
    "carry"  t[N] != 0 after the last iteration (the subtraction is decided by the carry),
    "ge"     no carry and t >= m (decided by the borrow alone),
    "lt"     t < m (no subtraction),
and the operands launched are exactly the operands the model saw.  What is reachable follows from the loop invariant
t <= a + m - 1 at the top of every iteration:
    spill needs a 2^32 + m - 1 >= 2^(32 (N + 1)) for some a < m, i.e. (m - 1)(2^32 + 1) >= 2^(32 (N + 1)): only moduli within 2^-32
    of 2^(32 N) (the "largest" prime and 2^(2l) - 1 of the fixture; the standard primes 2^(2l) - c are of this kind);
    carry needs ((m - 1)^2 + (R - 1) m) / R >= R (m above 0.618 R): never for a modulus just above 2^(2l - 1);
    ge and lt are reachable for every modulus.
Witnesses for carry / ge / lt are searched with integers on the CPU and added to the launch, so every reachable event is
executed on the device, and an event that cannot occur is asserted never to occur in the model."""
import json
import os
import random

import pytest

import orc_generic as OG

FIX = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "bign_generic_adv.json")))
MASK = 0xFFFFFFFF
EVENTS = ("spill", "carry", "ge", "lt")


def n0_of(m):
    return (-pow(m, -1, 1 << 32)) & MASK


def cios_model(a, b, m, N):
    """g_mul word by word: the same rows, the same carries, the same final selection.  Returns (result, events)."""
    A = [(a >> (32 * i)) & MASK for i in range(N)]
    Pm = [(m >> (32 * i)) & MASK for i in range(N)]
    n0 = n0_of(m)
    t = [0] * (N + 2)
    ev = set()
    for i in range(N):
        bi = (b >> (32 * i)) & MASK
        c = 0
        for j in range(N):
            s = A[j] * bi + t[j] + c
            t[j], c = s & MASK, s >> 32
        s = t[N] + c
        t[N], t[N + 1] = s & MASK, s >> 32
        if t[N + 1]:
            ev.add("spill")
        mm = (t[0] * n0) & MASK
        s = mm * Pm[0] + t[0]
        assert s & MASK == 0
        c = s >> 32
        for j in range(1, N):
            s = mm * Pm[j] + t[j] + c
            t[j - 1], c = s & MASK, s >> 32
        s = t[N] + c
        t[N - 1] = s & MASK
        t[N] = t[N + 1] + (s >> 32)
        assert t[N] <= 1                                   # t < 2 m < 2^(32 N + 1): the kernel keeps this word in 32 bits
    tv = sum(w << (32 * i) for i, w in enumerate(t[:N]))
    borrow = tv < m
    if t[N]:
        ev.add("carry")
    elif not borrow:
        ev.add("ge")
    else:
        ev.add("lt")
    r = (tv + (t[N] << (32 * N)) - m) if (t[N] or not borrow) else tv
    assert r == a * b * pow(1 << (32 * N), -1, m) % m, (hex(a), hex(b), hex(m))
    return r, ev


def final_event(a, b, m, N):
    """which of carry / ge / lt the product ends in, from integers alone (the witness search)"""
    R = 1 << (32 * N)
    t = (a * b + ((-a * b * pow(m, -1, R)) % R) * m) >> (32 * N)
    return "carry" if t >= R else "ge" if t >= m else "lt"


def possible(event, m, N):
    R = 1 << (32 * N)
    if event == "spill":
        return (m - 1) * ((1 << 32) + 1) >= R << 32
    if event == "carry":
        return ((m - 1) ** 2 + (R - 1) * m) // R >= R
    return True


def special_operands(m, N):
    R = 1 << (32 * N)
    ones = sum(MASK << (64 * i) for i in range(N // 2))              # all-ones in the even limbs
    vals = [0, 1, 2, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2, R % m, R * R % m, (R - 1) % m, 1 << (16 * N), (1 << (16 * N)) - 1,
            (1 << (32 * N - 1)) % m, ((1 << (32 * N - 1)) - 1) % m, ones % m, (ones << 32) % m, (R - 1 - (MASK << 32)) % m,
            MASK, MASK << (32 * (N - 1)) if MASK << (32 * (N - 1)) < m else (m >> 32 << 32), m - (1 << 32) if m > 1 << 33 else 3,
            (m - 1) & ~MASK | 1]
    out = []
    for v in vals:
        v %= m
        if v not in out:
            out.append(v)
    return out


def operand_pairs(m, N, seed, n_random_model=40, n_search=4000):
    """(pairs the word-level model runs on and the device gets, events they reach)"""
    rnd = random.Random(seed)
    sp = special_operands(m, N)
    pairs = [(a, b) for a in sp for b in sp]
    pairs += [(rnd.randrange(m), rnd.randrange(m)) for _ in range(n_random_model)]
    # integer search for the final events the directed pairs may miss; a found witness joins the launch
    need = {e for e in ("carry", "ge", "lt") if possible(e, m, N)}
    for a, b in pairs:
        need.discard(final_event(a, b, m, N))
    for _ in range(n_search):
        if not need:
            break
        a, b = rnd.randrange(m - (m >> 6), m), rnd.randrange(m - (m >> 6), m)
        e = final_event(a, b, m, N)
        if e in need:
            need.discard(e)
            pairs.append((a, b))
    if "ge" in need:
        w = ge_witness(m, N)
        if w:
            pairs.append(w)
    return pairs


def ge_witness(m, N):
    """a pair that ends in [m, R) when R - m is tiny (random pairs land there with probability (R - m) / R): the product ends in
    t = r + m with r < R - m exactly when a b = (r + m) R - (R - j) m = r R + j m for some j, so factor such numbers"""
    R = 1 << (32 * N)
    for r in range(min(R - m, 64)):
        for j in range(1, 64):
            X = r * R + j * m
            for f in range(r + j + 1, 2000):
                if X % f == 0 and X // f < m:
                    assert final_event(f, X // f, m, N) == "ge"
                    return f, X // f
    return None


def coverage(m, N, pairs):
    counts = dict.fromkeys(EVENTS, 0)
    want = []
    for a, b in pairs:
        r, ev = cios_model(a, b, m, N)
        want.append(r)
        for e in ev:
            counts[e] += 1
    return want, counts


def check_coverage(mod, counts, N):
    m = OG.le(bytes.fromhex(mod["m"]))
    for e in EVENTS:
        if possible(e, m, N):
            assert counts[e] > 0, f"{e} is reachable for the {mod['kind']} modulus of l = {mod['l']} and no operand pair reached it"
        else:
            assert counts[e] == 0, f"{e} cannot occur for the {mod['kind']} modulus of l = {mod['l']}, yet the model saw it"


def is_probable_prime(n):
    """Miller-Rabin, plain Python: the first 24 primes as bases (deterministic far beyond 64 bits, 2^-48 beyond)"""
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89)
    for q in small:
        if n % q == 0:
            return n == q
    d, r = n - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    for base in small:
        x = pow(base, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(r - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


# ------------------------------------------------------------------------------------------------------ CPU
def test_fixture_moduli_have_the_shapes_they_are_named_for():
    """every committed p is a 2l-bit prime = 3 (mod 4) (Miller-Rabin here, not trusted from the tool), every q an odd 2l-bit
    number, and the limb patterns are what the kinds say -- n0 = 1 and n0 = 0xFFFFFFFF included"""
    for l in (128, 192, 256):
        mods = [x for x in FIX["moduli"] if x["l"] == l]
        assert [x["kind"] for x in mods] == ["smallest", "largest", "low limb ffffffff", "low limb 3", "interior zero limb",
                                              "interior ones limb", "random", "2^(2l) - 1", "2^(2l-1) + 1", "low limb 1", "random odd"]
        N = l // 16
        by = {x["kind"]: OG.le(bytes.fromhex(x["m"])) for x in mods}
        for x in mods:
            m = by[x["kind"]]
            assert m >> (2 * l - 1) == 1 and m & 1
            if x["prime"]:
                assert m % 4 == 3 and is_probable_prime(m), (l, x["kind"])
        p = by["smallest"] - 4
        while p >> (2 * l - 1):
            assert not (p % 4 == 3 and is_probable_prime(p))
            p -= 4
        p = by["largest"] + 4
        while p >> (2 * l) == 0:
            assert not (p % 4 == 3 and is_probable_prime(p))
            p += 4
        limb = lambda v, j: (v >> (32 * j)) & MASK
        assert limb(by["low limb ffffffff"], 0) == MASK and n0_of(by["low limb ffffffff"]) == 1
        assert limb(by["low limb 3"], 0) == 3
        assert limb(by["low limb 1"], 0) == 1 and n0_of(by["low limb 1"]) == MASK
        assert limb(by["interior zero limb"], N // 2) == 0 and limb(by["interior ones limb"], N // 2) == MASK
        assert by["2^(2l) - 1"] == (1 << (2 * l)) - 1 and by["2^(2l-1) + 1"] == (1 << (2 * l - 1)) + 1
    for s in FIX["sets"]:
        assert is_probable_prime(OG.le(bytes.fromhex(s["p"]))), s["p_kind"]
        assert OG.params_check(OG.Params.from_hex(s)) == 0


def test_every_reachable_branch_of_the_cios_loop_is_reached_by_the_operands():
    """the reachability condition of the module docstring, on the CPU, for the operand pairs the GPU test launches"""
    seen = {(l, e): 0 for l in (128, 192, 256) for e in EVENTS}
    for mi, mod in enumerate(FIX["moduli"]):
        N = mod["l"] // 16
        m = OG.le(bytes.fromhex(mod["m"]))
        _, counts = coverage(m, N, operand_pairs(m, N, mi))
        check_coverage(mod, counts, N)
        for e in EVENTS:
            seen[mod["l"], e] += counts[e]
        if mod["kind"] in ("largest", "2^(2l) - 1"):
            assert counts["spill"] > 0 and counts["carry"] > 0
        if mod["kind"] in ("smallest", "2^(2l-1) + 1"):
            assert counts["spill"] == 0 and counts["carry"] == 0 and counts["ge"] > 0
    for (l, e), c in seen.items():
        assert c > 0, f"{e} is unreachable for every modulus of l = {l}"


def test_five_newton_steps_already_give_n0():
    """the host code runs six steps x <- x (2 - p0 x) from x = 1; the error exponent doubles from one correct bit, so five
    are exact for every odd p0 and six change nothing (which is why dropping ONE step is not a detectable change; dropping
    two is, and the moduli with low limb 3 and 0xFFFFFFFF show it)"""
    def newton(p0, steps):
        x = 1
        for _ in range(steps):
            x = (x * (2 - p0 * x)) & MASK
        return x
    rnd = random.Random(5)
    for p0 in [1, 3, 5, 7, MASK, MASK - 2, 0x80000001, 0x7FFFFFFF] + [rnd.getrandbits(32) | 1 for _ in range(2000)]:
        assert newton(p0, 5) == newton(p0, 6) == pow(p0, -1, 1 << 32)
    low = [OG.le(bytes.fromhex(mod["m"])) & MASK for mod in FIX["moduli"]]
    assert 3 in low and MASK in low and all(newton(p0, 4) != pow(p0, -1, 1 << 32) for p0 in (3, MASK))


# ------------------------------------------------------------------------------------------------------ GPU
def _run(eng, l, op, m, vals_a, vals_b, width=1, a=None, b=None):
    """one hook call over lists of integers (width = limbs groups per item: 1 field element, 3 a point)"""
    import torch
    from gpulib import dev, host
    no = l // 4
    n = len(vals_a) // width
    ta = dev(b"".join(v.to_bytes(no, "little") for v in vals_a))
    tb = dev(b"".join(v.to_bytes(no, "little") for v in vals_b)) if vals_b is not None else None
    out = torch.zeros(len(vals_a) * no, dtype=torch.uint8, device="cuda")
    pad = lambda v: None if v is None else v.to_bytes(no, "little") + bytes(64 - no)
    code = eng.debug_feG(l, op, pad(m), pad(a), pad(b), ta, tb, out, n)
    assert code == 0, (l, op, code)
    torch.cuda.synchronize()
    raw = host(out)
    return [OG.le(raw[no * i: no * i + no]) for i in range(len(vals_a))]


@pytest.mark.gpu
def test_generic_field_ops_match_python_integers_on_every_modulus():
    """g_mul = a b R^-1, g_add, g_sub, x R and x R^-1 on all pairs of the special operands, the witnesses and 3000 random pairs per
    modulus, with the context of make_mod and (op | 0x100) of make_curve; the word-level model vouches that the rare branches ran"""
    from gpulib import exp_engine
    eng = exp_engine()
    for mi, mod in enumerate(FIX["moduli"]):
        l = mod["l"]
        N = l // 16
        m = OG.le(bytes.fromhex(mod["m"]))
        R = 1 << (32 * N)
        Ri = pow(R, -1, m)
        pairs = operand_pairs(m, N, mi)
        want, counts = coverage(m, N, pairs)
        check_coverage(mod, counts, N)
        rnd = random.Random(1000 + mi)
        more = [(rnd.randrange(m), rnd.randrange(m)) for _ in range(3000)]
        A = [x for x, _ in pairs + more]
        B = [y for _, y in pairs + more]
        want += [x * y * Ri % m for x, y in more]
        for flag in (0, 0x100):
            if flag and not mod["prime"]:
                continue                                    # make_curve is the builder of p; the odd q's go through make_mod as in the product
            tag = (l, mod["kind"], flag)
            got = _run(eng, l, 0 | flag, m, A, B)
            bad = [(hex(x), hex(y)) for x, y, g, w in zip(A, B, got, want) if g != w]
            assert not bad, (tag, "g_mul", len(bad), bad[:3])
            got = _run(eng, l, 1 | flag, m, A, B)
            assert got == [(x + y) % m for x, y in zip(A, B)], (tag, "g_add")
            got = _run(eng, l, 2 | flag, m, A, B)
            assert got == [(x - y) % m for x, y in zip(A, B)], (tag, "g_sub")
            got = _run(eng, l, 4 | flag, m, A, None)
            assert got == [x * R % m for x in A], (tag, "to Montgomery")
            got = _run(eng, l, 5 | flag, m, A, None)
            assert got == [x * Ri % m for x in A], (tag, "from Montgomery")


@pytest.mark.gpu
def test_generic_inversion_matches_python_integers_on_every_prime():
    """g_inv(a R) = a^(p-2) R (Montgomery in and out) and 0 for 0, on the special operands and random ones"""
    from gpulib import exp_engine
    eng = exp_engine()
    for mi, mod in enumerate(FIX["moduli"]):
        if not mod["prime"]:
            continue
        l = mod["l"]
        N = l // 16
        m = OG.le(bytes.fromhex(mod["m"]))
        R = 1 << (32 * N)
        rnd = random.Random(2000 + mi)
        A = special_operands(m, N) + [rnd.randrange(m) for _ in range(200)]
        got = _run(eng, l, 3, m, A, None)
        assert got[0] == 0
        assert got == [pow(x, m - 2, m) * R * R % m for x in A], (l, mod["kind"])


def _points(P, rnd):
    """the affine points of the cases: P, -P, 2P, Q and the point of order 2 where the set has one"""
    no = P.l // 4
    p, a, yG = OG.le(P.p[:no]), OG.le(P.a[:no]), OG.le(P.yG[:no])
    G = (0, yG)
    Pt = OG.mul(rnd.getrandbits(64) | 1, G, a, p)
    Q = OG.mul(rnd.getrandbits(P.l) | 1, G, a, p)
    return p, a, [Pt, (Pt[0], p - Pt[1]), OG._add(Pt, Pt, a, p), Q]


def _affine_pairs(pts):
    return [(x, y) for x in [None] + pts for y in [None] + pts]


@pytest.mark.gpu
def test_generic_jacobian_doubling_and_addition_match_the_affine_group_law():
    """gj_add(T, E) and gj_dbl(T) on all ordered pairs from {O, P, -P, 2P, Q, the point of order 2}, every finite point as
    (x, y, 1) and as (x z^2, y z^3, z) with a random z, O as (junk, junk, 0): T == E with different Z falls into the doubling,
    T == -E gives O, doubling a point with Y == 0 gives O.  The checker is orc_generic._add on affine points."""
    from gpulib import exp_engine
    eng = exp_engine()
    for si, s in enumerate(FIX["sets"]):
        P = OG.Params.from_hex(s)
        l = P.l
        no = l // 4
        rnd = random.Random(3000 + si)
        p, a, pts = _points(P, rnd)
        if "x0" in s:
            pts.append((OG.le(bytes.fromhex(s["x0"])), 0))
            assert OG._add(pts[-1], pts[-1], a, p) is None
        R = 1 << (8 * no)

        def jac(pt, z):
            if pt is None:
                return [rnd.randrange(p), rnd.randrange(p), 0]
            return [pt[0] * z * z % p * R % p, pt[1] * z * z * z % p * R % p, z * R % p]

        def aff(X, Y, Z):
            if Z == 0:
                return None
            Ri = pow(R, -1, p)
            X, Y, Z = X * Ri % p, Y * Ri % p, Z * Ri % p
            zi = pow(Z, p - 2, p)
            return X * zi * zi % p, Y * zi * zi * zi % p

        TA, TB, want, names = [], [], [], []
        for x, y in _affine_pairs(pts):
            for zx in (1, rnd.randrange(2, p)):
                for zy in (1, rnd.randrange(2, p)):
                    TA += jac(x, zx)
                    TB += jac(y, zy)
                    want.append(OG._add(x, y, a, p))
                    names.append((x, y, zx == 1, zy == 1))
        assert any(x == y and x is not None for x, y, _, _ in names)
        got = _run(eng, l, 7, OG.le(P.p[:no]), TA, TB, width=3, a=a)
        bad = [nm for i, nm in enumerate(names) if aff(*got[3 * i: 3 * i + 3]) != want[i]]
        assert not bad, (si, s["kind"], s["p_kind"], "gj_add", len(bad), bad[:2])
        TA, want = [], []
        for x in [None] + pts:
            for z in (1, rnd.randrange(2, p), rnd.randrange(2, p)):
                TA += jac(x, z)
                want.append(OG._add(x, x, a, p))
        got = _run(eng, l, 6, OG.le(P.p[:no]), TA, None, width=3, a=a)
        assert [aff(*got[3 * i: 3 * i + 3]) for i in range(len(want))] == want, (si, s["kind"], s["p_kind"], "gj_dbl")


@pytest.mark.gpu
def test_generic_complete_addition_matches_the_affine_group_law_on_odd_order_curves():
    """gp_add_complete (Renes-Costello-Batina, general a) on the same pairs, homogeneous coordinates (x z, y z, z), O as
    (0, y, 0); and the in-place doubling the ladder uses.  ONLY on the isomorphic images of the standard curves: the formulas
    are complete for groups of odd order, which is what tools/model_rcb_general.py models; on a curve with a point of order 2
    they have exceptional pairs (P - Q of order 2) and nothing is claimed or tested there."""
    from gpulib import exp_engine
    eng = exp_engine()
    isos = [(si, s) for si, s in enumerate(FIX["sets"]) if s["kind"] == "iso"]
    assert {s["l"] for _, s in isos} == {128, 192, 256}
    for si, s in isos:
        P = OG.Params.from_hex(s)
        l = P.l
        no = l // 4
        rnd = random.Random(4000 + si)
        p, a, pts = _points(P, rnd)
        b = OG.le(P.b[:no])
        R = 1 << (8 * no)

        def proj(pt, z):
            if pt is None:
                return [0, z * R % p, 0]
            return [pt[0] * z % p * R % p, pt[1] * z % p * R % p, z * R % p]

        def aff(X, Y, Z):
            if Z == 0:
                assert X == 0 and Y != 0
                return None
            zi = pow(Z, p - 2, p)
            return X * zi % p, Y * zi % p

        TA, TB, want = [], [], []
        for x, y in _affine_pairs(pts):
            for zx in (1, rnd.randrange(2, p)):
                for zy in (1, rnd.randrange(2, p)):
                    TA += proj(x, zx)
                    TB += proj(y, zy)
                    want.append(OG._add(x, y, a, p))
        got = _run(eng, l, 8, p, TA, TB, width=3, a=a, b=b)
        assert [aff(*got[3 * i: 3 * i + 3]) for i in range(len(want))] == want, (si, "gp_add_complete")
        TA, want = [], []
        for x in [None] + pts:
            for z in (1, rnd.randrange(2, p)):
                TA += proj(x, z)
                want.append(OG._add(x, x, a, p))
        got = _run(eng, l, 9, p, TA, None, width=3, a=a, b=b)
        assert [aff(*got[3 * i: 3 * i + 3]) for i in range(len(want))] == want, (si, "gp_add_complete in place")
