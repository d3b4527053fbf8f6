// TEST INFRASTRUCTURE: a C view of bee2_amd/csrc/belt_kwp_common.hpp -- the per-lane transform of belt_kwp_batch_kernel, the
// slab layout and the launch plan -- so that tests/test_beltkwp.py can pin the kernel's own text to the model on the CPU: the
// transform runs on a [dword][64] array with the host belt of host_small.hpp.  Built by the test itself: g++ -O2 -shared
// -fPIC, no sanitizer flags.  Nothing here ships.
#include <string.h>
#include "../../bee2_amd/csrc/belt_kwp_common.hpp"
#include "../../bee2_amd/csrc/host_small.hpp"

using namespace bee2hip;
using namespace bee2hip::hostp;
static BeltTables g_T;

namespace {
constexpr uint32_t DW_MAX = KWP_TOKEN_MAX / 4;
struct Column {
    uint32_t (*slab)[64];
    uint32_t lane;
    uint32_t ld(uint32_t j) const { return slab[j][lane]; }
    void st(uint32_t j, uint32_t v) { slab[j][lane] = v; }
};
struct HostEK {
    const uint32_t *key;
    void operator()(uint32_t (&x)[4]) const { belt_encr(g_T, x, key); }
};
}  // namespace

extern "C" {
void hk_init(const uint8_t H[256]) { belt_tables(g_T, H); }

// One record through kwp_lane in column `lane` of a slab whose every other octet -- the other 63 columns, the pad octets of
// this one, the dwords past the token -- holds a pattern made from `seed`.  in: T - 16 octets (wrap) or T (unwrap); out: T
// (wrap) or T - 16 (unwrap); hdr: 16 octets or null.  Returns the transform's code, or 0xFFFFFFFF when a dword of another
// column or past the token changed.
uint32_t hk_lane(int unwrap, uint32_t T, const uint32_t key[8], const uint8_t *hdr, const uint8_t *in, uint8_t *out, uint32_t lane,
                 uint32_t seed)
{
    static uint32_t slab[DW_MAX][64], before[DW_MAX][64];
    uint32_t z = seed | 1u;
    for (uint32_t j = 0; j < DW_MAX; ++j)
        for (uint32_t l = 0; l < 64; ++l) { z ^= z << 13; z ^= z >> 17; z ^= z << 5; slab[j][l] = z; }
    uint8_t *octets = reinterpret_cast<uint8_t *>(slab);
    const uint32_t in_len = unwrap ? T : T - 16, out_len = unwrap ? T - 16 : T;
    for (uint32_t b = 0; b < in_len; ++b) octets[kwp_slab_octet(T, lane, b)] = in[b];
    memcpy(before, slab, sizeof slab);
    uint32_t h[4] = {0, 0, 0, 0};
    if (hdr)
        for (int k = 0; k < 4; ++k) h[k] = ld32le(hdr + 4 * k);
    Column col{slab, lane};
    HostEK ek{key};
    const uint32_t code = kwp_lane(col, ek, T, unwrap ? 1u : 0u, h);
    for (uint32_t b = 0; b < out_len; ++b) out[b] = octets[kwp_slab_octet(T, lane, b)];
    for (uint32_t j = 0; j < DW_MAX; ++j)
        for (uint32_t l = 0; l < 64; ++l)
            if ((l != lane || j >= kwp_dwords(T)) && slab[j][l] != before[j][l]) return 0xFFFFFFFFu;
    return code;
}

void hk_plan(uint32_t T, uint32_t out[3])
{
    const KwpPlan p = kwp_plan(T);
    out[0] = p.waves; out[1] = p.wave_bytes; out[2] = p.lds;
}
uint32_t hk_pad(uint32_t T) { return kwp_pad(T); }
uint32_t hk_dwords(uint32_t T) { return kwp_dwords(T); }
}
