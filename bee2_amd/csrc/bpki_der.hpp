// bpki_der.hpp -- the two DER frames of STB 34.101.78's password-protected containers (src/crypto/bpki.c:66-305 of bee2):
// EncryptedPrivateKeyInfo (PBES2 / PBKDF2 with hmac-hbelt / belt-kwp256) around a belt-kwp token, and the PrivateKeyInfo inside
// the token, for a bign private key (24, 32, 48 or 64 octets) or a bels share (17, 25 or 33 octets).  A parser and a builder
// for each, written against the format; what is accepted is what bee2's der.c accepts (the notes at the functions say where
// that is more, or less, than one would guess).  Plain C++17, no HIP, no allocation: the product includes it (capi_bpki.hip) and
// the tests compile it with g++ as it stands (tests/hostshim/host_bpki_shim.cpp).
// The input is untrusted: every read is checked against the length first, lengths are compared as `need <= left` with `left`
// never above the buffer's length, and nothing is added to a length taken from the input before it has been so compared.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace bee2hip {
namespace bpki {

// object identifiers as arcs; the first element is the number of arcs
static const uint32_t OID_BIGN_PUBKEY[] = {11, 1, 2, 112, 0, 2, 0, 34, 101, 45, 2, 1};
static const uint32_t OID_BIGN_CURVE[4][12] = {{11, 1, 2, 112, 0, 2, 0, 34, 101, 45, 3, 0}, {11, 1, 2, 112, 0, 2, 0, 34, 101, 45, 3, 1},
                                               {11, 1, 2, 112, 0, 2, 0, 34, 101, 45, 3, 2}, {11, 1, 2, 112, 0, 2, 0, 34, 101, 45, 3, 3}};
static const uint32_t OID_BELS_SHARE[] = {10, 1, 2, 112, 0, 2, 0, 34, 101, 60, 11};
static const uint32_t OID_BELS_M0[3][12] = {{11, 1, 2, 112, 0, 2, 0, 34, 101, 60, 2, 1}, {11, 1, 2, 112, 0, 2, 0, 34, 101, 60, 2, 2},
                                            {11, 1, 2, 112, 0, 2, 0, 34, 101, 60, 2, 3}};
static const uint32_t OID_PBES2[] = {7, 1, 2, 840, 113549, 1, 5, 13};
static const uint32_t OID_PBKDF2[] = {7, 1, 2, 840, 113549, 1, 5, 12};
static const uint32_t OID_BELT_KWP256[] = {10, 1, 2, 112, 0, 2, 0, 34, 101, 31, 73};
static const uint32_t OID_HMAC_HBELT[] = {10, 1, 2, 112, 0, 2, 0, 34, 101, 47, 12};

constexpr size_t PRIVKEY_LENS[4] = {24, 32, 48, 64};
constexpr size_t SHARE_LENS[3] = {17, 25, 33};
constexpr size_t KEY_MAX = 64;

// ------------------------------------------------------------------------------------------------ reading
struct Reader {
    const uint8_t *p;
    size_t len, pos;
    size_t left() const { return len - pos; }                  // pos <= len always

    // tag octet + length field (der.c derTDec / derLDec): a one-octet tag equal to `tag` (every tag of the two frames is one);
    // the length definite and minimal -- 0x80 and 0xFF refused, the long form with no leading zero octet, not for a value below
    // 128, at most 8 octets, not 2^64 - 1 -- and the value inside the buffer
    bool tl(uint8_t tag, size_t *vlen)
    {
        if (left() < 2 || p[pos] != tag) return false;
        const uint8_t l0 = p[pos + 1];
        if (l0 == 0x80 || l0 == 0xFF) return false;
        uint64_t l = l0;
        size_t used = 2;
        if (l0 > 0x80) {
            const size_t r = l0 - 0x80u;
            if (r > 8 || left() - 2 < r || p[pos + 2] == 0 || (r == 1 && p[pos + 2] < 128)) return false;
            l = 0;
            for (size_t k = 0; k < r; ++k) l = l << 8 | p[pos + 2 + k];
            if (l == UINT64_MAX) return false;
            used += r;
        }
        if (l > left() - used) return false;
        pos += used;
        *vlen = (size_t)l;
        return true;
    }
    // SEQUENCE: -> the position its content must end at (derTSEQDecStart does not compare the length with the buffer and
    // derTSEQDecStop wants the content to end exactly there; as nothing here reads past the buffer the two agree)
    bool seq(size_t *end)
    {
        size_t l;
        if (!tl(0x30, &l)) return false;
        *end = pos + l;
        return true;
    }
    bool stop(size_t end) const { return pos == end; }
    bool null()
    {
        size_t l;
        return tl(0x05, &l) && l == 0;
    }
    // OCTET STRING: -> where its octets are
    bool oct(size_t *off, size_t *vlen)
    {
        if (!tl(0x04, vlen)) return false;
        *off = pos;
        pos += *vlen;
        return true;
    }
    // INTEGER that fits a size_t (derTSIZEDec): at most 9 octets, the first without its top bit, no zero octet in front that
    // is not needed, nine octets only with a zero in front.  bee2 takes an INTEGER of NO octets for 0 when the octet behind it
    // has its top bit clear; so does this, and a missing octet behind it is a refusal (something follows in both frames)
    bool size(uint64_t *val)
    {
        size_t l;
        if (!tl(0x02, &l) || l > 9) return false;
        if (l == 0) {
            if (left() < 1 || (p[pos] & 0x80)) return false;
            *val = 0;
            return true;
        }
        const uint8_t *v = p + pos;
        if ((v[0] & 0x80) || (v[0] == 0 && l > 1 && !(v[1] & 0x80)) || (l == 9 && v[0] != 0)) return false;
        uint64_t x = 0;
        for (size_t k = 0; k < l; ++k) x = x << 8 | v[k];
        *val = x;
        pos += l;
        return true;
    }
    // OBJECT IDENTIFIER equal to `oid` (derOIDDec2): arcs in base 128, no 0x80 in front of an arc, an arc refused once bits 25
    // and up are set before the next octet.  As in bee2, octets of an arc that never ends (top bits set up to the end of the
    // value) behind the last arc are not looked at: the loop compares an arc when it ends.
    bool oid(const uint32_t *want)
    {
        size_t l;
        if (!tl(0x06, &l)) return false;
        const uint8_t *v = p + pos;
        const uint32_t n = want[0];
        uint32_t val = 0, idx = 0;
        bool first = true;
        for (size_t k = 0; k < l; ++k) {
            if (val & 0xFE000000u) return false;
            if (val == 0 && v[k] == 0x80) return false;
            val = val << 7 | (v[k] & 127u);
            if (v[k] & 0x80) continue;
            if (first) {
                const uint32_t d1 = val < 40 ? 0 : val < 80 ? 1 : 2;
                val -= 40 * d1;
                if (idx >= n || want[1 + idx++] != d1) return false;
                first = false;
            }
            if (idx >= n || want[1 + idx++] != val) return false;
            val = 0;
        }
        if (idx != n) return false;
        pos += l;
        return true;
    }
};

// EncryptedPrivateKeyInfo (bpki.c:206-305, bpkiEdataDec) of exactly `len` octets
struct Epki {
    bool ok;
    uint8_t salt[8];
    uint64_t iter;
    size_t edata_off, edata_len;
};
static inline Epki epki_parse(const uint8_t *epki, size_t len)
{
    Epki r;
    memset(&r, 0, sizeof r);
    if (!epki) return r;
    Reader d{epki, len, 0};
    size_t e_epki, e_alg, e_pbes2, e_kdf, e_par, e_prf, e_kwp, o_salt, l_salt;
    if (!d.seq(&e_epki)) return r;
    if (!d.seq(&e_alg) || !d.oid(OID_PBES2)) return r;
    if (!d.seq(&e_pbes2)) return r;
    if (!d.seq(&e_kdf) || !d.oid(OID_PBKDF2)) return r;
    if (!d.seq(&e_par) || !d.oct(&o_salt, &l_salt) || l_salt != 8 || !d.size(&r.iter)) return r;
    if (!d.seq(&e_prf) || !d.oid(OID_HMAC_HBELT) || !d.null() || !d.stop(e_prf)) return r;
    if (!d.stop(e_par) || !d.stop(e_kdf)) return r;
    if (!d.seq(&e_kwp) || !d.oid(OID_BELT_KWP256) || !d.null() || !d.stop(e_kwp)) return r;
    if (!d.stop(e_pbes2) || !d.stop(e_alg)) return r;
    if (!d.oct(&r.edata_off, &r.edata_len) || !d.stop(e_epki) || d.pos != len) return r;
    memcpy(r.salt, epki + o_salt, 8);
    r.ok = true;
    return r;
}

// PrivateKeyInfo (bpki.c:66-204, bpkiPrivkeyDec / bpkiShareDec) of exactly `len` octets; kind 0 = a bign private key, 1 = a
// bels share.  -> the key's length with the key copied to key[0 .. KEY_MAX) (zeros behind it), or 0
static inline size_t pki_parse(int kind, const uint8_t *pki, size_t len, uint8_t key[KEY_MAX])
{
    memset(key, 0, KEY_MAX);
    if (!pki) return 0;
    Reader d{pki, len, 0};
    size_t e_pki, e_alg, off, l, want = 0;
    uint64_t version;
    if (!d.seq(&e_pki) || !d.size(&version) || version != 0) return 0;
    if (!d.seq(&e_alg) || !d.oid(kind ? OID_BELS_SHARE : OID_BIGN_PUBKEY)) return 0;
    const size_t mark = d.pos;
    for (size_t k = 0; k < (kind ? 3u : 4u) && !want; ++k) {
        d.pos = mark;
        if (d.oid(kind ? OID_BELS_M0[k] : OID_BIGN_CURVE[k])) want = kind ? SHARE_LENS[k] : PRIVKEY_LENS[k];
    }
    if (!want || !d.stop(e_alg)) return 0;
    if (!d.oct(&off, &l) || l != want || !d.stop(e_pki) || d.pos != len) return 0;
    memcpy(key, pki + off, want);
    return want;
}

// ------------------------------------------------------------------------------------------------ writing
// Sizes first, octets second: every function returns the octets of its element and writes them when out is not null.
static inline size_t der_len_octets(size_t l)
{
    size_t r = 1;
    if (l >= 128)
        for (; l; l >>= 8) ++r;
    return r;
}
static inline size_t put_tl(uint8_t *out, uint8_t tag, size_t l)
{
    const size_t c = der_len_octets(l);
    if (out) {
        out[0] = tag;
        if (c == 1) out[1] = (uint8_t)l;
        else {
            out[1] = (uint8_t)(0x80 | (c - 1));
            for (size_t k = c - 1; k >= 1; --k, l >>= 8) out[1 + k] = (uint8_t)l;
        }
    }
    return 1 + c;
}
static inline size_t put_oid(uint8_t *out, const uint32_t *oid)
{
    uint8_t v[64];
    size_t l = 0;
    for (uint32_t k = 1; k < oid[0]; ++k) {
        const uint32_t arc = k == 1 ? 40 * oid[1] + oid[2] : oid[1 + k];
        size_t c = 1;
        for (uint32_t t = arc >> 7; t; t >>= 7) ++c;
        for (size_t j = 0; j < c; ++j) v[l + j] = (uint8_t)((arc >> (7 * (c - 1 - j)) & 127u) | (j + 1 < c ? 0x80u : 0u));
        l += c;
    }
    const size_t tl = put_tl(out, 0x06, l);
    if (out) memcpy(out + tl, v, l);
    return tl + l;
}
static inline size_t put_size(uint8_t *out, uint64_t val)
{
    size_t l = 1;
    for (uint64_t v = val; v >= 256; v >>= 8) ++l;
    if (val >> (8 * (l - 1)) & 0x80) ++l;                      // a zero octet in front of a set top bit
    const size_t tl = put_tl(out, 0x02, l);
    if (out)
        for (size_t k = 0; k < l; ++k) out[tl + k] = l - 1 - k >= 8 ? 0 : (uint8_t)(val >> (8 * (l - 1 - k)));
    return tl + l;
}
static inline size_t put_null(uint8_t *out) { return put_tl(out, 0x05, 0); }
static inline uint8_t *adv(uint8_t *out, size_t n) { return out ? out + n : nullptr; }

// bpkiPrivkeyEnc / bpkiShareEnc: key_len is one of the kind's lengths (else 0 comes back); key may be null with out null
static inline size_t pki_build(uint8_t *out, int kind, const uint8_t *key, size_t key_len)
{
    const uint32_t *params = nullptr;
    for (size_t k = 0; k < (kind ? 3u : 4u); ++k)
        if (key_len == (kind ? SHARE_LENS[k] : PRIVKEY_LENS[k])) params = kind ? OID_BELS_M0[k] : OID_BIGN_CURVE[k];
    if (!params) return 0;
    const uint32_t *alg = kind ? OID_BELS_SHARE : OID_BIGN_PUBKEY;
    const size_t l_alg = put_oid(nullptr, alg) + put_oid(nullptr, params);
    const size_t l_pki = put_size(nullptr, 0) + put_tl(nullptr, 0x30, l_alg) + l_alg + put_tl(nullptr, 0x04, key_len) + key_len;
    size_t c = put_tl(out, 0x30, l_pki);
    c += put_size(adv(out, c), 0);
    c += put_tl(adv(out, c), 0x30, l_alg);
    c += put_oid(adv(out, c), alg);
    c += put_oid(adv(out, c), params);
    c += put_tl(adv(out, c), 0x04, key_len);
    if (out) memcpy(out + c, key, key_len);
    return c + key_len;
}

// bpkiEdataEnc: -> the container's length; with out not null the frame is written and *edata_off says where the edata_len
// octets of the token go -- they are copied from edata when that is not null, else left to the caller
static inline size_t epki_build(uint8_t *out, const uint8_t salt[8], uint64_t iter, const uint8_t *edata, size_t edata_len,
                                size_t *edata_off)
{
    const size_t l_prf = put_oid(nullptr, OID_HMAC_HBELT) + put_null(nullptr);
    const size_t l_par = put_tl(nullptr, 0x04, 8) + 8 + put_size(nullptr, iter) + put_tl(nullptr, 0x30, l_prf) + l_prf;
    const size_t l_kdf = put_oid(nullptr, OID_PBKDF2) + put_tl(nullptr, 0x30, l_par) + l_par;
    const size_t l_kwp = put_oid(nullptr, OID_BELT_KWP256) + put_null(nullptr);
    const size_t l_pbes2 = put_tl(nullptr, 0x30, l_kdf) + l_kdf + put_tl(nullptr, 0x30, l_kwp) + l_kwp;
    const size_t l_alg = put_oid(nullptr, OID_PBES2) + put_tl(nullptr, 0x30, l_pbes2) + l_pbes2;
    const size_t l_epki = put_tl(nullptr, 0x30, l_alg) + l_alg + put_tl(nullptr, 0x04, edata_len) + edata_len;
    size_t c = put_tl(out, 0x30, l_epki);
    c += put_tl(adv(out, c), 0x30, l_alg);
    c += put_oid(adv(out, c), OID_PBES2);
    c += put_tl(adv(out, c), 0x30, l_pbes2);
    c += put_tl(adv(out, c), 0x30, l_kdf);
    c += put_oid(adv(out, c), OID_PBKDF2);
    c += put_tl(adv(out, c), 0x30, l_par);
    c += put_tl(adv(out, c), 0x04, 8);
    if (out) memcpy(out + c, salt, 8);
    c += 8;
    c += put_size(adv(out, c), iter);
    c += put_tl(adv(out, c), 0x30, l_prf);
    c += put_oid(adv(out, c), OID_HMAC_HBELT);
    c += put_null(adv(out, c));
    c += put_tl(adv(out, c), 0x30, l_kwp);
    c += put_oid(adv(out, c), OID_BELT_KWP256);
    c += put_null(adv(out, c));
    c += put_tl(adv(out, c), 0x04, edata_len);
    if (edata_off) *edata_off = c;
    if (out && edata) memcpy(out + c, edata, edata_len);
    return c + edata_len;
}

}  // namespace bpki
}  // namespace bee2hip
