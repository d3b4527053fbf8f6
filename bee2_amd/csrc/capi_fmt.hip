// capi_fmt.hip -- belt-fmt, format-preserving encryption (STB 34.101.31; src/crypto/belt/belt_fmt.c): the batch over n records
// of one (mod, count) and the two bee2 one-shots.  Part of the C ABI (capi.hip), after capi_beltae.hip.  One record = one lane
// of belt_fmt_batch_kernel (belt_fmt_kernels.hip); a single record on the host is host_fmt.hpp.
#include "host_fmt.hpp"

// what the batch entries refuse before any device work
static err_t beltfmt_check(int decr, u32 mod, size_t count, const octet key[], size_t key_len, size_t n)
{
    if (decr != 0 && decr != 1) return ERR_BAD_INPUT;
    if (mod < 2 || mod > FMT_MOD_MAX || count < 2) return ERR_BAD_INPUT;
    if ((key_len != 16 && key_len != 24 && key_len != 32) || !key) return ERR_BAD_INPUT;
    if (n > 0xffffffffull) return ERR_BAD_INPUT;
    if (count > FMT_COUNT_MAX) return ERR_NOT_IMPLEMENTED;           // as bee2 (belt_fmt.c:435)
    return ERR_OK;
}

extern "C" err_t bee2hip_beltFMT_batch_stream(int decr, u32 mod, size_t count, const octet key[], size_t key_len,
                                              const void *d_ivs, const void *d_src, size_t n, void *d_dst, void *stream)
try {
    err_t code = beltfmt_check(decr, mod, count, key, key_len, n);
    if (code != ERR_OK) return code;
    if (n && (!d_src || !d_dst)) return ERR_BAD_INPUT;
    if (misaligned(d_src, 2) || misaligned(d_dst, 2)) return ERR_BAD_INPUT;
    if (n == 0) return ERR_OK;
    if (partly_overlap(d_src, d_dst, n * count * 2)) return ERR_BAD_INPUT;
    code = ensure_device();
    if (code != ERR_OK) return code;
    u32 kw[8];
    beltKeyExpand2(kw, key, key_len);
    code = launch_belt_fmt_batch(decr, mod, count, kw, host_beltH(), d_ivs, d_src, n, d_dst, as_stream(stream));
    wipe_host(kw, sizeof kw);
    return code;
} B2H_CATCH

// one Stage: the records once, processed in place on the device (as beltae_host)
extern "C" err_t bee2hip_beltFMT_batch(int decr, u32 mod, size_t count, const octet key[], size_t key_len, const octet *ivs,
                                       const u16 *src, size_t n, u16 *dst)
try {
    const err_t code = beltfmt_check(decr, mod, count, key, key_len, n);
    if (code != ERR_OK) return code;
    if (n && (!src || !dst)) return ERR_BAD_INPUT;
    if (n == 0) return ERR_OK;
    const size_t bytes = n * count * 2;
    Stage sg(3, false, "bee2hip_beltFMT staging");
    const size_t o_rec = sg.add(bytes), o_iv = sg.add(ivs ? n * 16 : 0);
    B2H_OK(sg.open(16));
    B2H_OK(sg.in(o_rec, src, bytes));
    if (ivs) B2H_OK(sg.in(o_iv, ivs, n * 16));
    B2H_OK(bee2hip_beltFMT_batch_stream(decr, mod, count, key, key_len, ivs ? sg.at(o_iv) : nullptr, sg.at(o_rec), n,
                                        sg.at(o_rec), nullptr));
    return sg.out(dst, o_rec, bytes);
} B2H_CATCH

// ---- bee2's one-shots (belt_fmt.c:422-476)
static err_t fmt_oneshot(int decr, u16 dest[], u32 mod, const u16 src[], size_t count, const octet key[], size_t len,
                         const octet iv[16], const char *what)
{
    if (count < 2 || !key_len_ok(len) || !src || !key || !dest) return ERR_BAD_INPUT;
    if (iv) {                                                        // dest and iv must be disjoint (belt_fmt.c:433)
        const uintptr_t d = (uintptr_t)dest, v = (uintptr_t)iv;
        if (d < v + 16 && v < d + 2 * count) return ERR_BAD_INPUT;
    }
    if (mod < 2 || mod > FMT_MOD_MAX) return ERR_BAD_INPUT;          // bee2 asserts
    if (count > FMT_COUNT_MAX) return ERR_NOT_IMPLEMENTED;
    return with_host(K_SERIAL, 2 * count, what, [&]() -> err_t {
        Stage sg(1, false, "beltFMT staging");
        const size_t o_rec = sg.add(2 * count), o_iv = sg.add(16);
        B2H_OK(sg.open(16));
        B2H_OK(sg.in(o_rec, src, 2 * count));
        if (iv) B2H_OK(sg.in(o_iv, iv, 16));
        B2H_OK(bee2hip_beltFMT_batch_stream(decr, mod, count, key, len, iv ? sg.at(o_iv) : nullptr, sg.at(o_rec), 1,
                                            sg.at(o_rec), nullptr));
        return sg.out(dest, o_rec, 2 * count);
    }, [&] {
        u32 kw[8];
        beltKeyExpand2(kw, key, len);
        if (dest != src) memmove(dest, src, 2 * count);
        hostp::fmt_crypt(hostT(), decr, mod, count, kw, host_beltH(), iv, dest);
        wipe_host(kw, sizeof kw);
    });
}

extern "C" err_t beltFMTEncr(u16 dest[], u32 mod, const u16 src[], size_t count, const octet key[], size_t len, const octet iv[16])
try {
    return fmt_oneshot(0, dest, mod, src, count, key, len, iv, "beltFMTEncr");
} B2H_CATCH

extern "C" err_t beltFMTDecr(u16 dest[], u32 mod, const u16 src[], size_t count, const octet key[], size_t len, const octet iv[16])
try {
    return fmt_oneshot(1, dest, mod, src, count, key, len, iv, "beltFMTDecr");
} B2H_CATCH
