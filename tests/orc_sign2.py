"""TEST INFRASTRUCTURE: the one-time key of bignSign2 (STB 34.101.45 algorithm 6.3.3, bign_sign.c:195-217) restated in
Python over an ARBITRARY q, and bignSign2 on top of it (orc_generic.sign_k does the rest).

    theta = belt-hash(oid || d || t);   k <- H;   k <- belt-wbl_theta(k)  until 0 < k < q

Every pass is a whole belt-wbl encryption of 2l bits with its round counter starting again at 1 (beltWBLStepE sets
st->round = 0, belt_wbl.c:203).  On the standard curves the first pass is rejected with probability below 2^-126; on a
parameter set whose q sits anywhere in [2^(2l-1), 2^(2l)) up to one pass in two is.  belt-hash and belt-wbl come from the
C oracle (orclib) or, in the fixture's tool, from the reference.  Pinned by tests/test_sign2_model.py against
tests/golden/bign_sign2_nonce.json, which the reference produced (tools/make_golden_sign2_nonce.py)."""
import orc_generic as OG

ERR_OK, ERR_BAD_PRIVKEY = 0, 504


def nonce(oid_der, d, t, h, q, belt_hash, wbl, max_passes=4096):
    """(k, passes): d, h octet strings of 2l bits, t octets or None (the same as empty), q an integer; wbl(msg, key) ->
    (code, msg') is ONE belt-wbl encryption.  k is an integer, passes >= 1."""
    theta = belt_hash(bytes(oid_der) + bytes(d) + bytes(t or b""))
    k = bytes(h)
    for passes in range(1, max_passes + 1):
        code, k = wbl(k, theta)
        assert code == 0
        if 0 < OG.le(k) < q:
            return OG.le(k), passes
    raise AssertionError("no one-time key in %d passes" % max_passes)


def sign2(P, oid_der, h, d, t, belt_hash, wbl):
    """bignSign2 (bign_sign.c:140-245): ERR_BAD_PRIVKEY unless 0 < d < q, then bignSign's tail with the k of 6.3.3.
    Returns (code, sig)."""
    code = OG.params_check(P)
    if code:
        return code, b""
    no = P.l // 4
    q = OG.le(P.q[:no])
    if not 0 < OG.le(d[:no]) < q:
        return ERR_BAD_PRIVKEY, b""
    k, _ = nonce(oid_der, d[:no], t, h[:no], q, belt_hash, wbl)
    return OG.sign_k(P, oid_der, h, d, k.to_bytes(no, "little"), belt_hash)


def recover_k(l, q, sig, d, h):
    """the one-time key behind a signature: s1 = k - (s0 + 2^l) d - H (mod q), so k = s1 + (s0 + 2^l) d + H (mod q) -- whatever
    R and s0 were.  sig, d, h octets; returns an integer in [0, q)."""
    no = l // 4
    s0, s1 = OG.le(sig[:no // 2]), OG.le(sig[no // 2:no // 2 + no])
    return (s1 + (s0 + (1 << l)) * OG.le(d[:no]) + OG.le(h[:no])) % q
