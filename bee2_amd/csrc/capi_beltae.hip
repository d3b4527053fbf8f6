// capi_beltae.hip -- belt-dwp / belt-che over ragged batches of records (STB 34.101.31; src/crypto/belt/belt_dwp.c, belt_che.c).
// Part of the C ABI (capi.hip), after capi_prg.hip.  One record = one lane of
// belt_ae_ragged_kernel (belt_ae_kernels.hip).  bee2's step functions stay what capi_belt.hip makes of them: one long stream.

// what beltDWPWrap / beltCHEWrap refuse (belt_che.c:263) plus the limits of one launch; before any device work
static err_t beltae_check(int mode, const octet key[], size_t key_len, size_t n)
{
    if (mode != 0 && mode != 1) return ERR_BAD_INPUT;
    if ((key_len != 16 && key_len != 24 && key_len != 32) || !key) return ERR_BAD_INPUT;
    if (n > 0xffffffffull) return ERR_BAD_INPUT;
    return ERR_OK;
}

extern "C" err_t bee2hip_beltAE_ragged_stream(int unwrap, int mode, const octet key[], size_t key_len, const void *d_ivs,
                                              const void *d_hdrs, const void *d_hdr_offsets, const void *d_src,
                                              const void *d_offsets, const void *d_order, size_t n, void *d_dst, void *d_tags,
                                              void *d_codes, void *stream)
try {
    err_t code = beltae_check(mode, key, key_len, n);
    if (code != ERR_OK) return code;
    if (unwrap != 0 && unwrap != 1) return ERR_BAD_INPUT;
    if (misaligned(d_offsets, 8) || misaligned(d_hdr_offsets, 8) || misaligned(d_order, 4) || misaligned(d_codes, 4))
        return ERR_BAD_INPUT;
    if (d_hdrs && !d_hdr_offsets) return ERR_BAD_INPUT;
    if ((d_src == nullptr) != (d_dst == nullptr)) return ERR_BAD_INPUT;
    if (n && (!d_offsets || !d_tags || !d_ivs || (unwrap && !d_codes))) return ERR_BAD_INPUT;
    if (n == 0) return ERR_OK;
    code = ensure_device();
    if (code != ERR_OK) return code;
    BeltAeArgs A;
    memset(&A, 0, sizeof A);
    beltKeyExpand2(A.key.k, key, key_len);
    const octet *H = host_beltH();
    for (int k = 0; k < 4; ++k) A.t0[k] = load32le(H + 4 * k);
    A.mode = (uint32_t)mode;
    A.unwrap = (uint32_t)unwrap;
    return launch_belt_ae_ragged(A, d_ivs, d_hdrs, d_hdr_offsets, d_src, d_offsets, d_order, n, d_dst, d_tags, d_codes,
                                 as_stream(stream));
} B2H_CATCH

// ---- host-pointer entries, as prg_ae_host: stage through t_scr[3] (staging.hpp: the ragged part of a Stage), the text once and
// processed in place, longest record first, one call of the stream entry on the NULL stream
static err_t beltae_host(int unwrap, int mode, const octet key[], size_t key_len, const octet *ivs, const octet *hdrs,
                         const uint64_t *hdr_offsets, const octet *src, const uint64_t *offsets, size_t n, octet *dst, octet *tags,
                         err_t *codes)
{
    err_t code = beltae_check(mode, key, key_len, n);
    if (code != ERR_OK) return code;
    if (n == 0) return ERR_OK;
    if (!offsets || !tags || !ivs || (unwrap && !codes) || (hdrs && !hdr_offsets)) return ERR_BAD_INPUT;
    if (!offsets_rise(offsets, n) || (hdr_offsets && !offsets_rise(hdr_offsets, n))) return ERR_BAD_INPUT;
    Stage sg(3, false, "bee2hip_beltAE staging");
    RaggedPart txt(sg, offsets, n), hdr(sg, hdr_offsets, n);
    if ((txt.total && (!src || !dst)) || (hdr.total && !hdrs)) return ERR_BAD_INPUT;
    std::vector<uint32_t> ord;
    longest_first(ord, offsets, n);
    const size_t o_iv = sg.add(n * 16);
    txt.add_offs(sg);
    hdr.add_offs(sg);
    const size_t o_ord = sg.add(n * 4), o_tag = sg.add(n * 8), o_code = sg.add(n * 4);
    B2H_OK(sg.open(16));
    B2H_OK(txt.in(sg, src));
    B2H_OK(hdr.in(sg, hdrs));
    B2H_OK(sg.in(o_iv, ivs, n * 16));
    if (unwrap) B2H_OK(sg.in(o_tag, tags, n * 8));
    B2H_OK(sg.in(o_ord, ord.data(), n * 4));
    // in place on the device: the text is staged once
    B2H_OK(bee2hip_beltAE_ragged_stream(unwrap, mode, key, key_len, sg.at(o_iv), hdr.data(sg), hdr.offs(sg), txt.data(sg), txt.offs(sg),
                                        sg.at(o_ord), n, txt.data(sg), sg.at(o_tag), unwrap ? sg.at(o_code) : nullptr, nullptr));
    B2H_OK(txt.out(sg, dst));
    return unwrap ? sg.out(codes, o_code, n * 4) : sg.out(tags, o_tag, n * 8);
}

extern "C" err_t bee2hip_beltAE_wrap_ragged(int mode, const octet key[], size_t key_len, const octet *ivs, const octet *hdrs,
                                            const uint64_t *hdr_offsets, const octet *src, const uint64_t *offsets, size_t n,
                                            octet *dst, octet *tags)
try {
    return beltae_host(0, mode, key, key_len, ivs, hdrs, hdr_offsets, src, offsets, n, dst, tags, nullptr);
} B2H_CATCH

extern "C" err_t bee2hip_beltAE_unwrap_ragged(int mode, const octet key[], size_t key_len, const octet *ivs, const octet *hdrs,
                                              const uint64_t *hdr_offsets, const octet *src, const uint64_t *offsets, size_t n,
                                              const octet *tags, octet *dst, err_t *codes)
try {
    return beltae_host(1, mode, key, key_len, ivs, hdrs, hdr_offsets, src, offsets, n, dst, const_cast<octet *>(tags), codes);
} B2H_CATCH
