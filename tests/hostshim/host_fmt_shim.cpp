// TEST INFRASTRUCTURE: a C view of bee2_amd/csrc/host_fmt.hpp (the host path of beltFMTEncr / beltFMTDecr) and of
// belt_fmt_common.hpp (the block count, the division step the kernel shares) so that tests/test_beltfmt.py can pin them to the
// model on the CPU.  Built by the test itself: g++ -O2 -shared -fPIC, no sanitizer flags.  Nothing here ships.
#include "../../bee2_amd/csrc/host_fmt.hpp"

using namespace bee2hip;
using namespace bee2hip::hostp;
static BeltTables g_T;
static uint8_t g_H[256];

static uint64_t next64(uint64_t *s)          // splitmix64
{
    uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// (rem 2^16 + h) div / mod mod by fmt_divstep against the machine's own division; returns the number of differences
static uint64_t check_rem(uint32_t mod, uint32_t rem)
{
    const FmtDiv d = fmt_div_make(mod);
    uint64_t bad = 0;
    for (uint32_t h = 0; h < 65536; ++h) {
        const uint32_t cur = (rem << 16) | h;
        uint32_t q;
        const uint32_t r = fmt_divstep(rem, h, d, &q);
        bad += (q != cur / mod) || (r != cur % mod);
    }
    return bad;
}

extern "C" {
void hf_init(const uint8_t H[256])
{
    memcpy(g_H, H, 256);
    belt_tables(g_T, H);
}
void hf_crypt(int decr, uint32_t mod, size_t count, const uint32_t key[8], const uint8_t *iv, uint16_t *buf)
{
    fmt_crypt(g_T, decr, mod, count, key, g_H, iv, buf);
}
size_t hf_block_count(uint32_t mod, size_t n) { return fmt_block_count(mod, n); }
// the launch plan of belt_fmt_batch_kernel: b1, b2, num_bytes, wave_bytes, waves, lds
void hf_plan(uint32_t mod, size_t count, uint32_t out[6])
{
    const FmtPlan p = fmt_plan(mod, count);
    out[0] = p.b1; out[1] = p.b2; out[2] = p.num_bytes; out[3] = p.wave_bytes; out[4] = p.waves; out[5] = p.lds;
}
// every rem < mod and every h < 2^16
uint64_t hf_div_exhaustive(uint32_t mod)
{
    uint64_t bad = 0;
    for (uint32_t rem = 0; rem < mod; ++rem) bad += check_rem(mod, rem);
    return bad;
}
// every h with rem in {0, 1, mod / 2, mod - 2, mod - 1} and `extra` seeded values of rem
uint64_t hf_div_sampled(uint32_t mod, uint32_t extra, uint64_t seed)
{
    const uint32_t fixed[5] = {0, 1, mod / 2, mod - 2, mod - 1};
    uint64_t bad = 0;
    for (uint32_t rem : fixed) bad += check_rem(mod, rem);
    for (uint32_t i = 0; i < extra; ++i) bad += check_rem(mod, (uint32_t)(next64(&seed) % mod));
    return bad;
}
// fmt_divmod on the sums the mixing step forms: every t < 2^17
uint64_t hf_divmod_small(uint32_t mod)
{
    const FmtDiv d = fmt_div_make(mod);
    uint64_t bad = 0;
    for (uint32_t t = 0; t < (1u << 17); ++t) {
        uint32_t q;
        const uint32_t r = fmt_divmod(t, d, &q);
        bad += (q != t / mod) || (r != t % mod);
    }
    return bad;
}
}
