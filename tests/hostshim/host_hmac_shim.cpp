// TEST INFRASTRUCTURE: a C view of bee2_amd/csrc/belt_hmac_common.hpp -- hmac_lane(), the per-lane logic of
// belt_hmac_batch_kernel -- and of bee2_amd/csrc/host_hmac.hpp, the host path of beltHMAC / beltPBKDF2, so that
// tests/test_belthmac.py can pin both to the model on the CPU.  Built by the test itself: g++ -O2 -shared -fPIC, no sanitizer
// flags.  Nothing here ships.
#include <string.h>
#include "../../bee2_amd/csrc/belt_hmac_common.hpp"
#include "../../bee2_amd/csrc/host_hmac.hpp"

using namespace bee2hip;
using namespace bee2hip::hostp;
static BeltTables g_T;
static uint8_t g_H[256];

namespace {
// the reader the contract allows at its worst: the octets of X past cnt hold a pattern; cnt = 0 reads nothing; a block that
// reaches past its source, or cnt > 32, is counted
struct NoisyReader {
    const uint8_t *key, *msg;
    uint64_t key_len, msg_len;
    mutable uint32_t z, faults;
    void block(uint32_t (&X)[8], uint32_t is_key, uint64_t blk, uint32_t cnt) const
    {
        uint8_t b[32];
        for (int k = 0; k < 32; ++k) { z ^= z << 13; z ^= z >> 17; z ^= z << 5; b[k] = (uint8_t)(z >> 11); }
        if (cnt > 32 || (cnt && 32 * blk + cnt > (is_key ? key_len : msg_len))) { ++faults; return; }
        if (cnt) memcpy(b, (is_key ? key : msg) + 32 * blk, cnt);
        for (int k = 0; k < 8; ++k) X[k] = ld32le(b + 4 * k);
    }
};
}  // namespace

extern "C" {
void hh_init(const uint8_t H[256])
{
    memcpy(g_H, H, 256);
    belt_tables(g_T, H);
}

// One record through hmac_lane with the noisy reader.  shared = 1: the key's state is computed first (host_hmac.hpp, as a
// launch does) and the lane is given it instead of the key.  Returns the reader's fault count.
uint32_t hh_lane(uint32_t shared, const uint8_t *key, uint64_t key_len, const uint8_t *msg, uint64_t msg_len, uint32_t suffix,
                 uint32_t iter, uint32_t seed, uint8_t out[32])
{
    uint32_t H0[8], acc[8];
    for (int k = 0; k < 8; ++k) H0[k] = ld32le(g_H + 4 * k);
    HmacKeyState ks;
    memset(&ks, 0xA5, sizeof ks);
    if (shared) hmac_key_state(g_T, g_H, key, (size_t)key_len, ks);
    HmacHostCompress cf{g_T};
    NoisyReader rd{shared ? nullptr : key, msg, shared ? 0 : key_len, msg_len, seed | 1u, 0u};
    hmac_lane(cf, rd, H0, ks, shared, shared ? 0 : key_len, msg_len, suffix, iter, acc);
    for (int k = 0; k < 32; ++k) out[k] = (uint8_t)(acc[k >> 2] >> (8 * (k & 3)));
    return rd.faults;
}

// what the one-shots' host path runs (capi_hmac.hip): suffix 0 / iter 1 = beltHMAC, suffix 4 = beltPBKDF2
void hh_host(const uint8_t *key, uint64_t key_len, const uint8_t *msg, uint64_t msg_len, uint32_t suffix, uint32_t iter, uint8_t out[32])
{
    HmacKeyState ks;
    hmac_run(g_T, g_H, ks, 0, key, (size_t)key_len, msg, (size_t)msg_len, suffix, iter, out);
}

uint32_t hh_differs(const uint8_t a[32], const uint8_t b[32], uint32_t mac_len)
{
    uint32_t A[8], B[8];
    for (int k = 0; k < 8; ++k) { A[k] = ld32le(a + 4 * k); B[k] = ld32le(b + 4 * k); }
    return hmac_differs(A, B, mac_len);
}
}
