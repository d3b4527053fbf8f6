// host_fmt.hpp -- the HOST path of the drop-in beltFMTEncr / beltFMTDecr (product code; plain C++17, no HIP), beside
// host_small.hpp whose belt block function it uses and whose rules it follows: used only by the two bee2 one-shots, never by
// a batch entry.  One record is one serial chain of at least six E_K: a single call always runs here unless
// BEE2HIP_FORCE=gpu says otherwise.  An independent statement of belt_fmt.c:151-420 and belt_wbl.c:50-82 on 32-bit limbs;
// tests/test_beltfmt.py pins it to the model on the CPU, with and without sanitizers.
#pragma once
#include "belt_fmt_common.hpp"
#include "host_small.hpp"

namespace bee2hip {
namespace hostp {

// belt-32block (belt_fmt.c:157-175), belt-wbl encryption (belt_wbl.c:57-81; L limbs, L even, L >= 8) or one E_K on t[0 .. L)
static inline void fmt_cipher(const BeltTables &T, uint32_t *t, size_t L, const uint32_t key[8])
{
    if (L == 4) {
        belt_encr(T, t, key);
    } else if (L == 6) {
        static const unsigned bases[3] = {2, 4, 0};
        for (uint32_t r = 1; r <= 3; ++r) {
            const unsigned base = bases[r - 1];
            uint32_t x[4];
            for (unsigned k = 0; k < 4; ++k) x[k] = t[(base + k) % 6];
            belt_encr(T, x, key);
            x[0] ^= r;
            for (unsigned k = 0; k < 4; ++k) t[(base + k) % 6] = x[k];
            t[(base + 4) % 6] ^= x[0];
            t[(base + 5) % 6] ^= x[1];
        }
    } else {
        const uint32_t rounds = 2 * (uint32_t)((L + 3) / 4);
        for (uint32_t r = 1; r <= rounds; ++r) {
            uint32_t s[4] = {t[0], t[1], t[2], t[3]};
            for (size_t i = 4; i + 4 < L; i += 4)
                for (unsigned k = 0; k < 4; ++k) s[k] ^= t[i + k];
            memmove(t, t + 4, (L - 4) * sizeof(uint32_t));
            for (unsigned k = 0; k < 4; ++k) t[L - 4 + k] = s[k];
            belt_encr(T, s, key);
            s[0] ^= r;
            for (unsigned k = 0; k < 4; ++k) t[L - 8 + k] ^= s[k];
        }
    }
}

// buf: count symbols, processed in place; iv: 16 octets or null (zeros); H: beltH()
static inline void fmt_crypt(const BeltTables &T, int decr, uint32_t mod, size_t count, const uint32_t key[8], const uint8_t *H,
                             const uint8_t *iv, uint16_t *buf)
{
    const size_t n1 = (count + 1) / 2, n2 = count / 2;
    const size_t b1 = fmt_block_count(mod, n1), b2 = fmt_block_count(mod, n2);
    const FmtDiv D = fmt_div_make(mod);
    uint32_t ivx[6];
    ivx[0] = ivx[5] = (mod & 0xFFFFu) | (uint32_t)count << 16;
    for (int k = 0; k < 4; ++k) ivx[1 + k] = iv ? ld32le(iv + 4 * k) : 0u;
    std::vector<uint32_t> num(2 * (b1 > b2 ? b1 : b2) + 2);
    uint32_t *t = num.data();
    for (unsigned st = 0; st < 6; ++st) {
        const unsigned step = decr ? 5 - st : st;
        const bool second = (step & 1) != 0;
        const uint16_t *in = second ? buf : buf + n1;
        uint16_t *out = second ? buf + n1 : buf;
        const size_t in_cnt = second ? n1 : n2, out_cnt = second ? n2 : n1, b = second ? b1 : b2, nl = 2 * b, L = nl + 2;
        // Horner modulo 2^(64 b): a carry out of the top limb is dropped
        for (size_t j = 0; j < nl; ++j) t[j] = 0;
        for (size_t k = in_cnt; k-- > 0;) {
            uint64_t carry = in[k];
            for (size_t j = 0; j < nl; ++j) {
                const uint64_t p = (uint64_t)t[j] * mod + carry;
                t[j] = (uint32_t)p;
                carry = p >> 32;
            }
        }
        t[nl] = ld32le(H + 4 * step);
        t[nl + 1] = ivx[step];
        fmt_cipher(T, t, L, key);
        for (size_t k = 0; k < out_cnt; ++k) {
            uint32_t rem = 0;
            for (size_t j = L; j-- > 0;) {
                uint32_t qh, ql;
                rem = fmt_divstep(rem, t[j] >> 16, D, &qh);
                rem = fmt_divstep(rem, t[j] & 0xFFFFu, D, &ql);
                t[j] = qh << 16 | ql;
            }
            uint32_t q;
            out[k] = (uint16_t)fmt_divmod((uint32_t)out[k] + (decr ? mod - rem : rem), D, &q);
        }
    }
    for (size_t j = 0; j < num.size(); ++j) ((volatile uint32_t *)t)[j] = 0;
}

}  // namespace hostp
}  // namespace bee2hip
