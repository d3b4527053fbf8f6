// TEST INFRASTRUCTURE: the per-record-key form of belt_kwp_batch_kernel on the CPU -- kwp_key_words() and kwp_lane() of
// bee2_amd/csrc/belt_kwp_common.hpp, the text the kernel runs, over a whole [dword][64] slab: 64 records, 64 different keys, every
// lane its own E_K, with the host belt of host_small.hpp.  tests/test_bpki.py builds it: g++ -O2 -shared -fPIC, no sanitizer
// flags.  Nothing here ships.
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
struct LaneEK {
    const uint32_t (&K)[8];
    void operator()(uint32_t (&x)[4]) const { belt_encr(g_T, x, K); }
};
}  // namespace

extern "C" {
void hkk_init(const uint8_t H[256]) { belt_tables(g_T, H); }

// nrec <= 64 records as the kernel's wavefront sees them: record l in column l, its key the key_len octets keys + key_len * l
// (handed over at `keys_off` octets into a copy, so that every alignment is read), lanes past nrec under the zero key.
// in: nrec x (T - 16) (wrap) or nrec x T; out: nrec x T or nrec x (T - 16); codes: nrec (unwrap).  Returns 0, or 1 when a dword
// past the tokens changed.
uint32_t hkk_wave(int unwrap, uint32_t T, const uint8_t *keys, uint32_t key_len, uint32_t keys_off, const uint8_t *hdrs,
                  const uint8_t *in, uint32_t nrec, uint8_t *out, uint32_t *codes)
{
    static uint32_t slab[DW_MAX][64], before[DW_MAX][64];
    static uint8_t kbuf[64 * 32 + 8];
    uint32_t z = T | 1u;
    for (uint32_t j = 0; j < DW_MAX; ++j)
        for (uint32_t l = 0; l < 64; ++l) { z ^= z << 13; z ^= z >> 17; z ^= z << 5; slab[j][l] = z; }
    memcpy(before, slab, sizeof slab);
    memcpy(kbuf + (keys_off & 7u), keys, (size_t)key_len * nrec);
    uint8_t *octets = reinterpret_cast<uint8_t *>(slab);
    const uint32_t in_len = unwrap ? T : T - 16, out_len = unwrap ? T - 16 : T;
    for (uint32_t l = 0; l < nrec; ++l)
        for (uint32_t b = 0; b < in_len; ++b) octets[kwp_slab_octet(T, l, b)] = in[in_len * l + b];
    for (uint32_t l = 0; l < 64; ++l) {
        uint32_t K[8] = {0, 0, 0, 0, 0, 0, 0, 0}, h[4] = {0, 0, 0, 0};
        if (l < nrec) {
            kwp_key_words(K, kbuf + (keys_off & 7u) + (size_t)key_len * l, key_len);
            if (hdrs)
                for (int k = 0; k < 4; ++k) h[k] = ld32le(hdrs + 16 * l + 4 * k);
        }
        Column col{slab, l};
        LaneEK ek{K};
        const uint32_t code = kwp_lane(col, ek, T, unwrap ? 1u : 0u, h);
        if (unwrap && l < nrec) codes[l] = code;
    }
    for (uint32_t l = 0; l < nrec; ++l)
        for (uint32_t b = 0; b < out_len; ++b) out[out_len * l + b] = octets[kwp_slab_octet(T, l, b)];
    for (uint32_t j = kwp_dwords(T); j < DW_MAX; ++j)
        for (uint32_t l = 0; l < 64; ++l)
            if (slab[j][l] != before[j][l]) return 1;
    return 0;
}
}
