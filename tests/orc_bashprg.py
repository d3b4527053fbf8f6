"""TEST INFRASTRUCTURE: pure-Python restatement of the bash-prg automaton of STB 34.101.77 (src/crypto/bash/bash_prg.c:
start :110-136, commit :89-102, absorb :182-209, squeeze :228-255, encr :275-308, decr :328-361); bash-f comes from the C oracle
(orclib).  Pinned by tests/test_bashprg_model.py against tests/golden/bash_prg.json, which the reference itself produced
(tools/make_golden_bashprg.py)."""

ERR_OK, ERR_BAD_INPUT, ERR_BAD_PARAMS, ERR_BAD_MAC = 0, 109, 502, 511
NULL, KEY, DATA, TEXT, OUT = 0x01, 0x05, 0x09, 0x0D, 0x11
LD = ((128, 1), (128, 2), (192, 1), (192, 2), (256, 1), (256, 2))


def rate(l, d, keyed):
    """buf_len (bash_prg.c:133)"""
    return 192 - l * (2 + d) // 16 if keyed else 192 - d * l // 4


_bashF = None


def _F(state):
    global _bashF
    if _bashF is None:
        import orclib
        _bashF = orclib.load().bashF
    return bytearray(_bashF(bytes(state)))


class Prg:
    def __init__(self, l, d, ann=b"", key=b""):
        assert l in (128, 192, 256) and d in (1, 2)
        assert len(ann) % 4 == 0 and len(ann) <= 60 and len(key) % 4 == 0 and len(key) <= 60
        assert not key or len(key) >= l // 8
        self.l, self.d = l, d
        self.s = bytearray(192)
        self.s[0] = len(ann) * 4 + len(key) // 4
        self.s[1:1 + len(ann)] = ann
        self.s[1 + len(ann):1 + len(ann) + len(key)] = key
        self.pos = 1 + len(ann) + len(key)
        self.s[184] = l // 4 + d
        self.r = rate(l, d, bool(key))

    def commit(self, code):
        self.s[self.pos] ^= code
        self.s[self.r] ^= 0x80
        self.s = _F(self.s)
        self.pos = 0

    def _walk(self, data, fn):
        """fn(state octet, data octet) -> (new state octet, output octet), one octet at a time; bash-f whenever the buffer fills"""
        out = bytearray()
        for b in data:
            self.s[self.pos], o = fn(self.s[self.pos], b)
            out.append(o)
            self.pos += 1
            if self.pos == self.r:
                self.s = _F(self.s)
                self.pos = 0
        return bytes(out)

    def absorb(self, data):
        self.commit(DATA)
        self._walk(data, lambda s, b: (s ^ b, 0))

    def encr(self, data):
        self.commit(TEXT)
        return self._walk(data, lambda s, b: (s ^ b, s ^ b))

    def decr(self, data):
        self.commit(TEXT)
        return self._walk(data, lambda s, b: (b, s ^ b))

    def squeeze(self, n):
        self.commit(OUT)
        return self._walk(bytes(n), lambda s, b: (s, s))


def prg_hash(l, d, ann, msg, out_len):
    a = Prg(l, d, ann)
    a.absorb(msg)
    return a.squeeze(out_len)


def ae_wrap(l, d, key, ann, hdr, text, tag_len):
    a = Prg(l, d, ann, key)
    a.absorb(hdr)
    ct = a.encr(text)
    return ct, a.squeeze(tag_len)


def ae_unwrap(l, d, key, ann, hdr, ct, tag, tag_len=None):
    """-> (code, plaintext): zeros for a refused record, as the batch entries leave it"""
    a = Prg(l, d, ann, key)
    a.absorb(hdr)
    pt = a.decr(ct)
    if a.squeeze(len(tag) if tag_len is None else tag_len) != bytes(tag):
        return ERR_BAD_MAC, bytes(len(ct))
    return ERR_OK, pt


# ---- tests/golden/bash_prg.json: the random cases store seeds and lengths, not inputs
def case_inputs(c):
    """the inputs of a random fixture case, in this order from random.Random(c["seed"])"""
    import random
    rnd = random.Random(c["seed"])
    if c["kind"] == "hash":
        return {"ann": rnd.randbytes(c["ann_len"]), "msg": rnd.randbytes(c["msg_len"])}
    return {"key": rnd.randbytes(c["key_len"]), "ann": rnd.randbytes(c["ann_len"]), "hdr": rnd.randbytes(c["hdr_len"]),
            "text": rnd.randbytes(c["text_len"])}


def random_cases(seed, count):
    """parameters of `count` cases over all six (l, d): announcement 0 / 4 / 16 / 60, header and text lengths on and around
    the rate (and anywhere up to 400), key lengths l/8 .. 60, tag and digest lengths 1 / 8 / 32 / 64"""
    import random
    rnd = random.Random(seed)
    out = []
    for k in range(count):
        l, d = LD[k % 6]
        kind = "hash" if k % 3 == 0 else "ae"
        r = rate(l, d, kind == "ae")
        near = [0, 1, 3, 4, 5, r - 1, r, r + 1, 2 * r - 1, 2 * r, 2 * r + 1]
        pick = lambda: rnd.choice(near) if rnd.random() < 0.6 else rnd.randrange(0, 401)
        c = {"kind": kind, "l": l, "d": d, "seed": rnd.randrange(1 << 32), "ann_len": rnd.choice((0, 4, 16, 60))}
        if kind == "hash":
            c.update(msg_len=min(pick(), 400), out_len=rnd.choice((1, 8, 32, 64)))
        else:
            c.update(key_len=4 * rnd.randrange(l // 32, 16), hdr_len=min(pick(), 400), text_len=min(pick(), 400),
                     tag_len=rnd.choice((1, 8, 32, 64)))
        out.append(c)
    return out


def run_case(c, inputs=None):
    """what the model gives for a fixture case (vector or random): {"out"} or {"ct", "tag"} as hex"""
    x = inputs if inputs is not None else case_inputs(c)
    if c["kind"] == "hash":
        return {"out": prg_hash(c["l"], c["d"], x["ann"], x["msg"], c["out_len"]).hex()}
    ct, tag = ae_wrap(c["l"], c["d"], x["key"], x["ann"], x["hdr"], x["text"], c["tag_len"])
    return {"ct": ct.hex(), "tag": tag.hex()}
