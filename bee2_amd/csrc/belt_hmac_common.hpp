// belt_hmac_common.hpp -- what the kernel, the host path and the tests' CPU shim of belt-hmac / belt-pbkdf2 (STB 34.101.31;
// src/crypto/belt/belt_hmac.c, belt_pbkdf.c) share: one record's whole computation as a sequence of belt-compress steps, the
// padding and suffix masks, the length blocks.  Plain C++17: the tests compile it with g++ as it stands
// (tests/hostshim/host_hmac_shim.cpp) and run it with the host belt of host_small.hpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define B2H_HD __host__ __device__
#define B2H_UNROLL _Pragma("unroll")
#define B2H_ROLLED _Pragma("clang loop vectorize(disable) interleave(disable) unroll(disable)")
#else
#define B2H_HD
#define B2H_UNROLL
#define B2H_ROLLED
#endif

namespace bee2hip {

// iterations of one batch launch: its run time is proportional to them whatever n is -- 23 us an iteration, 3.1 s at this cap,
// 24.5 s at 2^20 (profiles/belt_hmac_rate.json) -- and the GPU may be shared
constexpr uint32_t HMAC_ITER_MAX = 1u << 17;
constexpr uint32_t HMAC_ERR_BAD_MAC = 511;      // err.h: ERR_BAD_MAC

// What a key leaves behind (belt_hmac.c:94-114): h / s after the block K0 ^ 36.. and after the block K0 ^ 5C.., both started
// from beltH()[0..32) and s = 0.  K0 = the key zero-padded to 32 octets, or its belt-hash when it is longer.
struct HmacKeyState { uint32_t hin[8], sin[4], hout[8], sout[4]; };

// the first cnt (0 .. 32) octets of a block stay, the rest becomes zero (the padding of belt-hash's last block)
B2H_HD static inline void hmac_keep(uint32_t (&X)[8], uint32_t cnt)
{
B2H_UNROLL
    for (uint32_t j = 0; j < 8; ++j) {
        const int32_t r = (int32_t)cnt - (int32_t)(4u * j);
        X[j] &= r >= 4 ? ~0u : r <= 0 ? 0u : (1u << (8 * r)) - 1u;
    }
}
// the closing block of a belt-hash of `octets` octets: <bit length as 128 bits> || s (belt_hash.c:120-135)
B2H_HD static inline void hmac_length_block(uint32_t (&X)[8], uint64_t octets, const uint32_t (&s)[4])
{
    X[0] = (uint32_t)(octets << 3); X[1] = (uint32_t)(octets >> 29); X[2] = (uint32_t)(octets >> 61); X[3] = 0;
B2H_UNROLL
    for (uint32_t k = 0; k < 4; ++k) X[4 + k] = s[k];
}
// 1 when the first mac_len (1 .. 32) octets of acc and M differ: every octet compared, no early exit
B2H_HD static inline uint32_t hmac_differs(const uint32_t (&acc)[8], const uint32_t (&M)[8], uint32_t mac_len)
{
    uint32_t D[8];
B2H_UNROLL
    for (uint32_t j = 0; j < 8; ++j) D[j] = acc[j] ^ M[j];
    hmac_keep(D, mac_len);
    uint32_t diff = 0;
B2H_UNROLL
    for (uint32_t j = 0; j < 8; ++j) diff |= D[j];
    return (diff | (0u - diff)) >> 31;
}

// The steps of one record.  Every step is ONE belt-compress; even steps absorb a block (s ^= s1), odd ones close a hash with
// its length block.  A lane walks them at its own pace: in a wavefront the lanes differ in key and message lengths, and all
// of them meet at the one compression site of the loop whatever step each is at.
enum : uint32_t {
    HS_KEY = 0,         // a block of a key longer than 32 octets (belt_hmac.c:59-89)
    HS_KEY_END = 1,     // ... its closing block: K0 = beltHash(key)
    HS_IPAD = 2,        // K0 ^ 36..: (h_in, s_in)
    HS_OPAD = 4,        // K0 ^ 5C..: (h_out, s_out)
    HS_MSG = 6,         // a block of the message (and of the suffix), the last one zero-padded
    HS_MSG_END = 7,     // the closing block of the inner hash: 256 + 8 (len + suffix) bits
    HS_OUT = 8,         // the inner digest as the second block of the outer hash
    HS_OUT_END = 9,     // the closing block of the outer hash: 512 bits
    HS_DONE = 10
};

// One record: acc = HMAC(key, msg || suffix) for iter = 1, and for iter > 1 the XOR of t_1 .. t_iter, t_1 = that MAC and
// t_k = HMAC(key, t_{k-1}) (belt_pbkdf.c:46-61).
//   cf(s1, h, X)                   belt-compress: s1 = sigma1, h = sigma2, both of (X, h)
//   rd.block(X, is_key, blk, cnt)  the cnt (0 .. 32) octets of block blk of the record's key (is_key) or message into the
//                                  front of X; the other octets of X may hold anything; cnt = 0 must not touch memory
//   H0                             beltH()[0..32) as words
//   shared                         the batch has one key and ks holds its state; else ks is computed here (and left in ks)
//   suffix                         0, or 4: the octets 00 00 00 01 follow the message (belt_pbkdf.c:50-51)
// shared, suffix and iter are the same for every record of a launch; lengths are not.  Nothing branches on, or is indexed by,
// an octet of a key, a message or a MAC: steps and masks follow lengths alone.
template <class CF, class RD>
B2H_HD static inline void hmac_lane(CF &cf, RD &rd, const uint32_t (&H0)[8], HmacKeyState &ks, const uint32_t shared,
                                    const uint64_t key_len, const uint64_t msg_len, const uint32_t suffix, const uint64_t iter,
                                    uint32_t (&acc)[8])
{
    const uint64_t total = msg_len + suffix;
    const uint64_t nmsg = (total + 31u) >> 5;           // blocks of msg || suffix, the partial one included
    uint32_t h[8], s[4] = {0, 0, 0, 0}, s1[4], X[8], K0[8];
    uint64_t blk = 0, nblk = nmsg;
    uint32_t step;
B2H_UNROLL
    for (uint32_t k = 0; k < 8; ++k) { h[k] = H0[k]; K0[k] = 0; }
    if (shared) {
B2H_UNROLL
        for (uint32_t k = 0; k < 8; ++k) h[k] = ks.hin[k];
B2H_UNROLL
        for (uint32_t k = 0; k < 4; ++k) s[k] = ks.sin[k];
        step = nmsg ? HS_MSG : HS_MSG_END;
    } else if (key_len > 32u) {
        nblk = (key_len + 31u) >> 5;
        step = HS_KEY;
    } else {
        rd.block(K0, 1u, 0, (uint32_t)key_len);
        hmac_keep(K0, (uint32_t)key_len);
        step = HS_IPAD;
    }
B2H_ROLLED
    while (step != HS_DONE) {
        if (step == HS_KEY || step == HS_MSG) {
            const uint32_t is_key = step == HS_KEY ? 1u : 0u;
            const uint64_t len = is_key ? key_len : msg_len, pos = blk << 5;
            const uint32_t cnt = pos >= len ? 0u : len - pos < 32u ? (uint32_t)(len - pos) : 32u;
            rd.block(X, is_key, blk, cnt);
            hmac_keep(X, cnt);
            if (!is_key && suffix) {
                // 00 00 00 01: three octets of the zero padding and the octet 01 at msg_len + 3, in whichever block that is
                const uint64_t q = msg_len + 3u - pos;                  // (wraps to >= 32 in the blocks behind it)
B2H_UNROLL
                for (uint32_t j = 0; j < 8; ++j)
                    X[j] |= (q >> 2) == j ? 1u << (8u * ((uint32_t)q & 3u)) : 0u;
            }
        } else if (step == HS_IPAD || step == HS_OPAD) {
            const uint32_t pad = step == HS_IPAD ? 0x36363636u : 0x5C5C5C5Cu;
B2H_UNROLL
            for (uint32_t k = 0; k < 8; ++k) { X[k] = K0[k] ^ pad; h[k] = H0[k]; }
B2H_UNROLL
            for (uint32_t k = 0; k < 4; ++k) s[k] = 0;
        } else if (step == HS_OUT) {
B2H_UNROLL
            for (uint32_t k = 0; k < 8; ++k) { X[k] = h[k]; h[k] = ks.hout[k]; }
B2H_UNROLL
            for (uint32_t k = 0; k < 4; ++k) s[k] = ks.sout[k];
        } else {
            hmac_length_block(X, step == HS_KEY_END ? key_len : step == HS_MSG_END ? total + 32u : 64u, s);
        }
        cf(s1, h, X);
        if (!(step & 1u)) {
B2H_UNROLL
            for (uint32_t k = 0; k < 4; ++k) s[k] ^= s1[k];
        }
        if (step == HS_KEY || step == HS_MSG) {
            if (++blk == nblk) step += 1u;
        } else if (step == HS_KEY_END) {
B2H_UNROLL
            for (uint32_t k = 0; k < 8; ++k) K0[k] = h[k];
            step = HS_IPAD;
        } else if (step == HS_IPAD) {
B2H_UNROLL
            for (uint32_t k = 0; k < 8; ++k) ks.hin[k] = h[k];
B2H_UNROLL
            for (uint32_t k = 0; k < 4; ++k) ks.sin[k] = s[k];
            step = HS_OPAD;
        } else if (step == HS_OPAD) {
B2H_UNROLL
            for (uint32_t k = 0; k < 8; ++k) { ks.hout[k] = h[k]; h[k] = ks.hin[k]; }
B2H_UNROLL
            for (uint32_t k = 0; k < 4; ++k) { ks.sout[k] = s[k]; s[k] = ks.sin[k]; }
            blk = 0; nblk = nmsg;
            step = nmsg ? HS_MSG : HS_MSG_END;
        } else {
            step = step == HS_MSG_END ? HS_OUT : step == HS_OUT ? HS_OUT_END : HS_DONE;
        }
    }
B2H_UNROLL
    for (uint32_t k = 0; k < 8; ++k) acc[k] = h[k];
    // t <- HMAC(key, t), acc ^= t: four compressions from the saved states, the second site.  j is the same in every lane.
B2H_ROLLED
    for (uint64_t j = 0; j < 4u * (iter - 1u); ++j) {
        const uint32_t q = (uint32_t)j & 3u;
        if (q & 1u) {
            hmac_length_block(X, 64u, s);
        } else {
B2H_UNROLL
            for (uint32_t k = 0; k < 8; ++k) { X[k] = h[k]; h[k] = q ? ks.hout[k] : ks.hin[k]; }
B2H_UNROLL
            for (uint32_t k = 0; k < 4; ++k) s[k] = q ? ks.sout[k] : ks.sin[k];
        }
        cf(s1, h, X);
        if (!(q & 1u)) {
B2H_UNROLL
            for (uint32_t k = 0; k < 4; ++k) s[k] ^= s1[k];
        }
        if (q == 3u) {
B2H_UNROLL
            for (uint32_t k = 0; k < 8; ++k) acc[k] ^= h[k];
        }
    }
}

}  // namespace bee2hip
