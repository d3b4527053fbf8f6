// host_hmac.hpp -- belt-hmac / belt-pbkdf2 of ONE record on the host (belt_hmac.c, belt_pbkdf.c): hmac_lane() of
// belt_hmac_common.hpp -- the kernel's own lane logic -- over host_small.hpp's belt_compress and a reader of host memory.  The
// path of the one-shots beltHMAC / beltPBKDF2 (a single record is one serial chain) and of the shared key's state, which a
// batch launch takes as an argument.
#pragma once
#include "belt_hmac_common.hpp"
#include "host_small.hpp"

namespace bee2hip {
namespace hostp {

struct HmacHostCompress {
    const BeltTables &T;
    void operator()(uint32_t (&s1)[4], uint32_t (&h)[8], const uint32_t (&X)[8]) const { belt_compress(T, s1, h, X); }
};
struct HmacHostReader {
    const uint8_t *key, *msg;
    void block(uint32_t (&X)[8], uint32_t is_key, uint64_t blk, uint32_t cnt) const
    {
        uint8_t b[32] = {0};
        if (cnt) memcpy(b, (is_key ? key : msg) + 32 * blk, cnt);
        for (int k = 0; k < 8; ++k) X[k] = ld32le(b + 4 * k);
        volatile uint8_t *w = b;
        for (int k = 0; k < 32; ++k) w[k] = 0;
    }
};

// out = the 32 octets of HMAC(key, msg || suffix) (iter = 1) or of PBKDF2's iteration over it; H = beltH().  shared: ks is
// the key's state and key is not read; else ks receives it.
static inline void hmac_run(const BeltTables &T, const uint8_t *H, HmacKeyState &ks, uint32_t shared, const uint8_t *key,
                            size_t key_len, const uint8_t *msg, size_t msg_len, uint32_t suffix, uint64_t iter, uint8_t out[32])
{
    uint32_t H0[8], acc[8];
    for (int k = 0; k < 8; ++k) H0[k] = ld32le(H + 4 * k);
    HmacHostCompress cf{T};
    HmacHostReader rd{key, msg};
    hmac_lane(cf, rd, H0, ks, shared, (uint64_t)key_len, (uint64_t)msg_len, suffix, iter, acc);
    for (int k = 0; k < 32; ++k) out[k] = (uint8_t)(acc[k >> 2] >> (8 * (k & 3)));
    volatile uint32_t *w = acc;
    for (int k = 0; k < 8; ++k) w[k] = 0;
}
// the state a key leaves behind: what a launch with one shared key is given
static inline void hmac_key_state(const BeltTables &T, const uint8_t *H, const uint8_t *key, size_t key_len, HmacKeyState &ks)
{
    uint8_t out[32];
    hmac_run(T, H, ks, 0, key, key_len, nullptr, 0, 0, 1, out);
}

}  // namespace hostp
}  // namespace bee2hip
