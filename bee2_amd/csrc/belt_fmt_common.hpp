// belt_fmt_common.hpp -- what the kernel, its launcher and the host path of belt-fmt (STB 34.101.31, format-preserving
// encryption; src/crypto/belt/belt_fmt.c) share: the block count b(mod, n) and the division step by the run-time modulus.
// Plain C++17: the tests compile it with g++ as it stands.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#if defined(__HIPCC__)
#define B2H_HD __host__ __device__
#else
#define B2H_HD
#endif

namespace bee2hip {

constexpr uint32_t FMT_MOD_MAX = 65536;
constexpr size_t FMT_COUNT_MAX = 600;

// The reciprocal of a modulus 2 <= mod <= 65536: rcp = floor(2^32 / mod) <= 2^31.
// For every t < 2^32, qe = floor(t rcp / 2^32) is floor(t / mod) or one less: t / mod - t rcp / 2^32 = t (2^32 / mod - rcp) / 2^32
// < t / 2^32 < 1, so ONE conditional correction makes quotient and remainder exact.  The products are 32 x 32 -> 64 bits
// (v_mul_hi_u32 on the device) and qe mod <= t: nothing can overflow, at the smallest modulus either.
struct FmtDiv { uint32_t mod, rcp; };
static inline FmtDiv fmt_div_make(uint32_t mod)
{
    return FmtDiv{mod, (uint32_t)(((uint64_t)1 << 32) / mod)};
}
// t = q mod + r, 0 <= r < mod, for any t < 2^32
B2H_HD static inline uint32_t fmt_divmod(uint32_t t, const FmtDiv d, uint32_t *q)
{
    const uint32_t qe = (uint32_t)(((uint64_t)t * d.rcp) >> 32);
    const uint32_t r = t - qe * d.mod;
    const uint32_t ge = r >= d.mod ? 1u : 0u;
    *q = qe + ge;
    return r - (ge ? d.mod : 0u);
}
// one step of the long division of a number held in 16-bit pieces, most significant first: (rem 2^16 + h) = q mod + rem',
// rem < mod and h < 2^16, hence q < 2^16.  Returns rem'.
B2H_HD static inline uint32_t fmt_divstep(uint32_t rem, uint32_t h, const FmtDiv d, uint32_t *q)
{
    return fmt_divmod((rem << 16) | h, d, q);
}

// b(mod, n): the smallest b with mod^n <= 2^(64 b), by exact integer arithmetic -- and the one pair at which bee2's own
// approximation (belt_fmt.c:74-149) gives one more, which is then part of the cipher: b(49667, 160) = 40, not 39.
static inline size_t fmt_block_count(uint32_t mod, size_t n)
{
    if (mod == 49667 && n == 160) return 40;
    std::vector<uint32_t> p(1, 1u);                              // mod^n, little-endian 32-bit limbs
    for (size_t i = 0; i < n; ++i) {
        uint64_t carry = 0;
        for (size_t j = 0; j < p.size(); ++j) {
            const uint64_t v = (uint64_t)p[j] * mod + carry;
            p[j] = (uint32_t)v;
            carry = v >> 32;
        }
        if (carry) p.push_back((uint32_t)carry);
    }
    for (size_t j = 0; j < p.size(); ++j)                       // mod^n - 1 (mod^n >= 2: no borrow out of the top)
        if (p[j]--) break;
    while (p.size() > 1 && p.back() == 0) p.pop_back();
    size_t bits = 32 * (p.size() - 1);
    for (uint32_t top = p.back(); top; top >>= 1) ++bits;
    const size_t b = (bits + 63) / 64;
    return b ? b : 1;
}

// How a launch is cut.  A wavefront owns its numbers -- [limb][lane] dwords, 2 max(b1, b2) + 2 limbs -- and then its 64
// records (128 count octets, 16-aligned); the S-box table sits in front of the wavefronts.  Four wavefronts per workgroup
// while two workgroups fit a CU's 160 KiB, else two, else one (at b = 75, count = 600 one wavefront owns 38 KiB of numbers
// and 75 KiB of records).
constexpr uint32_t FMT_TAB_BYTES = 4096;        // BeltTabSmall
struct FmtPlan { uint32_t b1, b2, num_bytes, wave_bytes, waves, lds; };
static inline FmtPlan fmt_plan(uint32_t mod, size_t count)
{
    FmtPlan p;
    p.b1 = (uint32_t)fmt_block_count(mod, (count + 1) / 2);
    p.b2 = (uint32_t)fmt_block_count(mod, count / 2);
    p.num_bytes = 256u * (2u * (p.b1 > p.b2 ? p.b1 : p.b2) + 2u);
    p.wave_bytes = p.num_bytes + (uint32_t)(128 * count);
    p.waves = 4;
    while (p.waves > 1 && FMT_TAB_BYTES + p.waves * p.wave_bytes > 80u * 1024u) p.waves >>= 1;
    p.lds = FMT_TAB_BYTES + p.waves * p.wave_bytes;
    return p;
}

// floor(log2(mod)): every division by mod takes at least this many bits off the number (the uniform trip counts of the kernel
// and the host path shrink with it)
static inline uint32_t fmt_floor_log2(uint32_t mod)
{
    uint32_t fl = 0;
    while ((mod >> (fl + 1)) != 0) ++fl;
    return fl;
}

}  // namespace bee2hip
