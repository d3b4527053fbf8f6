// belt_kwp_common.hpp -- what the kernel, its launcher and the tests' CPU shim of belt-kwp (STB 34.101.31, key wrap;
// src/crypto/belt/belt_kwp.c = belt-wbl, belt_wbl.c, over key || header) share: where a token's octets sit in a wavefront's
// slab, the per-lane transform between slab-in and slab-out, and the launch plan.  Plain C++17: the tests compile it with g++
// as it stands (tests/hostshim/host_kwp_shim.cpp) and run the transform on a [dword][64] array with the host belt.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define B2H_HD __host__ __device__
#define B2H_UNROLL _Pragma("unroll")
// a loop over the slab whose trip count is known only at run time: as written.  (Left alone, the compiler versions and
// interleaves these loops behind run-time overlap checks of the LDS addresses: twice the code, and scalar registers spilt.)
#define B2H_ROLLED _Pragma("clang loop vectorize(disable) interleave(disable) unroll(disable)")
#else
#define B2H_HD
#define B2H_UNROLL
#define B2H_ROLLED
#endif

namespace bee2hip {

constexpr uint32_t KWP_TOKEN_MAX = 1024;        // octets of a token: wrap count <= 1008, unwrap count <= 1024
constexpr uint32_t KWP_TOKEN_MIN = 32;
constexpr uint32_t KWP_TAB_BYTES = 4096;        // the S-box table in front of the slabs (BeltTabSmall)
constexpr uint32_t KWP_ERR_BAD_KEYTOKEN = 513;  // err.h: ERR_BAD_KEYTOKEN

// A token of T octets lives in its lane's slab column END-ALIGNED: `pad` = (4 - T mod 4) mod 4 octets of no meaning, then the
// token, so that octet b of the token is octet (pad + b) mod 4 of dword (pad + b) / 4 and the token ends with dword D - 1.
// belt-wbl works on the LAST two blocks of the buffer in every round (r* and the block before it) and kwp keeps its header
// in the last one: end-aligned, these are whole dwords for every T, and what straddles dwords when T mod 4 != 0 is the sum
// r1 + r2 + .. of the blocks counted from the FRONT.  That sum is formed as five dword columns and brought into place by
// one uniform funnel shift of 8 pad bits; the pad octets fall out of it, so they are never read into a result.
B2H_HD static inline uint32_t kwp_pad(uint32_t T) { return (0u - T) & 3u; }
B2H_HD static inline uint32_t kwp_dwords(uint32_t T) { return (T + 3u) >> 2; }
// the octet index, within a wavefront's slab of [dword][lane] dwords, of octet b of the token of lane l
B2H_HD static inline uint32_t kwp_slab_octet(uint32_t T, uint32_t l, uint32_t b)
{
    const uint32_t q = kwp_pad(T) + b;
    return ((q >> 2) * 64u + l) * 4u + (q & 3u);
}

// A record's own key: key_len = 16, 24 or 32 octets at q, any alignment, read octet by octet -> the eight words that
// beltKeyExpand2 makes of them (belt_lcl.c: 16 octets are repeated; 24 get k6 = k0 ^ k1 ^ k2 and k7 = k3 ^ k4 ^ k5).  key_len is
// uniform over a batch: no branch and no address depends on a key octet.
B2H_HD static inline void kwp_key_words(uint32_t (&K)[8], const uint8_t *q, uint32_t key_len)
{
    const uint32_t words = key_len >> 2;
B2H_UNROLL
    for (uint32_t k = 0; k < 8; ++k)
        K[k] = k < words ? (uint32_t)q[4 * k] | (uint32_t)q[4 * k + 1] << 8 | (uint32_t)q[4 * k + 2] << 16 | (uint32_t)q[4 * k + 3] << 24 : 0u;
    if (key_len == 16) {
B2H_UNROLL
        for (uint32_t k = 0; k < 4; ++k) K[4 + k] = K[k];
    } else if (key_len == 24) {
        K[6] = K[0] ^ K[1] ^ K[2];
        K[7] = K[3] ^ K[4] ^ K[5];
    }
}

// dword `lo` and the one above it, moved down by sh = 0, 8, 16 or 24 bits (v_alignbit_b32 on the device)
B2H_HD static inline uint32_t kwp_funnel(uint32_t lo, uint32_t hi, uint32_t sh)
{
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
}

// One token, in place in its slab column.  B.ld(j) / B.st(j, v) read and write dword j of the column, ek(x) is E_K on four
// words.  wrap (unwrap = 0): in = the key's `T - 16` octets, out = the token; the header hdr is put behind the key here.
// unwrap: in = the token, out = the key's T - 16 octets, or zeros when the header does not come out as hdr; returns ERR_OK or
// ERR_BAD_KEYTOKEN.  T, unwrap and hence every trip count and index are uniform over a batch; nothing branches on, or is
// indexed by, the key, a header or the data.
//
// A round of encryption (belt_wbl.c:57-81): s = the XOR of the blocks at octets 0, 16, .. while offset + 16 < T; the buffer
// moves down by 16 octets (four dwords, whatever T is), s becomes the last block and E_K(s) ^ <round> goes into the block
// before it.  Sum and move are one pass.  A round of decryption (belt_wbl.c:135-158) is that backwards: s = the last block,
// E_K(s) ^ <round> goes into the block before it, the buffer moves up, and the first block becomes s ^ the blocks at 16, 32 ..
// -- which after the move are the blocks at 0, 16, .. of before: again one pass.  (The block of the sum that reaches into the
// last 16 octets when T mod 16 != 0 must already hold E_K(s): hence the order.)  beltWBLStepD2, which kwp uses for the
// header, and StepD on the joined buffer are the same function, so one buffer serves.
template <class Slab, class EK>
B2H_HD static inline uint32_t kwp_lane(Slab &B, EK &ek, const uint32_t T, const uint32_t unwrap, const uint32_t (&hdr)[4])
{
    const uint32_t sh = 8u * kwp_pad(T), D = kwp_dwords(T);
    const uint32_t nb = (T - 1u) >> 4;                           // blocks in the sum: those with offset + 16 < T
    const uint32_t rounds = 2u * ((T + 15u) >> 4);
    if (!unwrap) {
B2H_UNROLL
        for (uint32_t m = 0; m < 4; ++m) B.st(D - 4 + m, hdr[m]);
    }
B2H_ROLLED
    for (uint32_t t = 1; t <= rounds; ++t) {
        const uint32_t round = unwrap ? rounds + 1u - t : t;
        uint32_t s[4];
        if (!unwrap) {
            // columns x[m] = XOR of dwords 4 k + m over the nb blocks, m = 0 .. 4 (the fifth = the first one without dword 0 and
            // with dword 4 nb), while everything moves down by four dwords
            uint32_t x[4];
B2H_UNROLL
            for (uint32_t m = 0; m < 4; ++m) x[m] = B.ld(m);
            const uint32_t edge = x[0] ^ B.ld(4u * nb);
            uint32_t blk = 4;
B2H_ROLLED
            for (; blk + 4 <= D; blk += 4) {
                uint32_t v[4];
B2H_UNROLL
                for (uint32_t m = 0; m < 4; ++m) v[m] = B.ld(blk + m);
                if (blk < 4u * nb) {
B2H_UNROLL
                    for (uint32_t m = 0; m < 4; ++m) x[m] ^= v[m];
                }
B2H_UNROLL
                for (uint32_t m = 0; m < 4; ++m) B.st(blk - 4 + m, v[m]);
            }
B2H_ROLLED
            for (; blk < D; ++blk) B.st(blk - 4, B.ld(blk));
            const uint32_t x4 = x[0] ^ edge;
            s[0] = kwp_funnel(x[0], x[1], sh);
            s[1] = kwp_funnel(x[1], x[2], sh);
            s[2] = kwp_funnel(x[2], x[3], sh);
            s[3] = kwp_funnel(x[3], x4, sh);
B2H_UNROLL
            for (uint32_t m = 0; m < 4; ++m) B.st(D - 4 + m, s[m]);
        } else {
B2H_UNROLL
            for (uint32_t m = 0; m < 4; ++m) s[m] = B.ld(D - 4 + m);
        }
        uint32_t e[4] = {s[0], s[1], s[2], s[3]};
        ek(e);
        e[0] ^= round;
B2H_UNROLL
        for (uint32_t m = 0; m < 4; ++m) B.st(D - 8 + m, B.ld(D - 8 + m) ^ e[m]);
        if (unwrap) {
            // everything moves up by four dwords, top first; the columns take the blocks 0 .. nb - 2 of before the move
            const uint32_t g = (D - 4u) >> 2;
            const uint32_t edge = nb >= 2 ? B.ld(0) ^ B.ld(4u * (nb - 1u)) : 0u;
B2H_ROLLED
            for (uint32_t j = D - 4u; j-- > 4u * g;) B.st(j + 4, B.ld(j));
            uint32_t x[4] = {0, 0, 0, 0};
B2H_ROLLED
            for (uint32_t k = g; k-- > 0;) {
                uint32_t v[4];
B2H_UNROLL
                for (uint32_t m = 0; m < 4; ++m) v[m] = B.ld(4 * k + m);
                if (k + 2 <= nb) {
B2H_UNROLL
                    for (uint32_t m = 0; m < 4; ++m) x[m] ^= v[m];
                }
B2H_UNROLL
                for (uint32_t m = 0; m < 4; ++m) B.st(4 * k + 4 + m, v[m]);
            }
            const uint32_t x4 = x[0] ^ edge;
            uint32_t w[4];
            w[0] = s[0] ^ kwp_funnel(x[0], x[1], sh);
            w[1] = s[1] ^ kwp_funnel(x[1], x[2], sh);
            w[2] = s[2] ^ kwp_funnel(x[2], x[3], sh);
            w[3] = s[3] ^ kwp_funnel(x[3], x4, sh);
            // the new first block starts `pad` octets into dword 0 and ends as many into dword 4, whose other octets stay
            B.st(0, kwp_funnel(0u, w[0], 32u - sh));
            B.st(1, kwp_funnel(w[0], w[1], 32u - sh));
            B.st(2, kwp_funnel(w[1], w[2], 32u - sh));
            B.st(3, kwp_funnel(w[2], w[3], 32u - sh));
            const uint32_t low = (uint32_t)(((uint64_t)1 << sh) - 1u);
            B.st(4, (B.ld(4) & ~low) | kwp_funnel(w[3], 0u, 32u - sh));
        }
    }
    if (!unwrap) return 0u;
    // all 16 octets of the header, no early exit; a refused token's key becomes zeros (belt_kwp.c:81-86)
    uint32_t diff = 0;
B2H_UNROLL
    for (uint32_t m = 0; m < 4; ++m) diff |= B.ld(D - 4 + m) ^ hdr[m];
    const uint32_t bad = (diff | (0u - diff)) >> 31;
    const uint32_t keep = bad - 1u;
B2H_ROLLED
    for (uint32_t j = 0; j + 4 < D; ++j) B.st(j, B.ld(j) & keep);
    return bad * KWP_ERR_BAD_KEYTOKEN;
}

// How a launch is cut: a wavefront owns ceil(T / 4) x 64 dwords of LDS; four wavefronts per workgroup while two workgroups
// (the table included) fit a CU's 160 KiB, else two, else one.
struct KwpPlan { uint32_t waves, wave_bytes, lds; };
static inline KwpPlan kwp_plan(uint32_t T)
{
    KwpPlan p;
    p.wave_bytes = 256u * kwp_dwords(T);
    p.waves = 4;
    while (p.waves > 1 && KWP_TAB_BYTES + p.waves * p.wave_bytes > 80u * 1024u) p.waves >>= 1;
    p.lds = KWP_TAB_BYTES + p.waves * p.wave_bytes;
    return p;
}

}  // namespace bee2hip
