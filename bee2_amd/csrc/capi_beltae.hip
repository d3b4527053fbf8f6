// capi_beltae.hip -- belt-dwp / belt-che over ragged batches of records (STB 34.101.31; src/crypto/belt/belt_dwp.c, belt_che.c).
// Part of the C ABI (capi.hip), after capi_prg.hip whose offset and ordering helpers it shares.  One record = one lane of
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

// ---- host-pointer entries, as prg_ae_host: stage through t_scr[3], the text once and processed in place, staged data keeps its
// alignment mod 16, longest record first, one call of the stream entry on the NULL stream
static err_t beltae_host(int unwrap, int mode, const octet key[], size_t key_len, const octet *ivs, const octet *hdrs,
                         const uint64_t *hdr_offsets, const octet *src, const uint64_t *offsets, size_t n, octet *dst, octet *tags,
                         err_t *codes)
{
    err_t code = beltae_check(mode, key, key_len, n);
    if (code != ERR_OK) return code;
    if (n == 0) return ERR_OK;
    if (!offsets || !tags || !ivs || (unwrap && !codes) || (hdrs && !hdr_offsets)) return ERR_BAD_INPUT;
    if (!prg_offsets_ok(offsets, n) || (hdr_offsets && !prg_offsets_ok(hdr_offsets, n))) return ERR_BAD_INPUT;
    const size_t first = (size_t)offsets[0], total = (size_t)(offsets[n] - offsets[0]);
    const size_t hfirst = hdr_offsets ? (size_t)hdr_offsets[0] : 0, htotal = hdr_offsets ? (size_t)(hdr_offsets[n] - hdr_offsets[0]) : 0;
    if ((total && (!src || !dst)) || (htotal && !hdrs)) return ERR_BAD_INPUT;
    std::vector<uint32_t> ord;
    prg_longest_first(ord, offsets, n);
    const size_t lead = first & 15, hlead = hfirst & 15;
    Stage sg(3, false, "bee2hip_beltAE staging");
    const size_t o_txt = sg.add(lead + total), o_hdr = sg.add(hlead + htotal), o_iv = sg.add(n * 16), o_off = sg.add((n + 1) * 8),
                 o_hoff = sg.add((n + 1) * 8), o_ord = sg.add(n * 4), o_tag = sg.add(n * 8), o_code = sg.add(n * 4);
    B2H_OK(sg.open(16));
    std::vector<uint64_t> off(n + 1);
    for (size_t i = 0; i <= n; ++i) off[i] = offsets[i] - first + lead;
    B2H_OK(sg.in(o_off, off.data(), (n + 1) * 8));
    if (hdr_offsets) {
        for (size_t i = 0; i <= n; ++i) off[i] = hdr_offsets[i] - hfirst + hlead;
        B2H_OK(sg.in(o_hoff, off.data(), (n + 1) * 8));
        if (htotal) B2H_OK(sg.in(o_hdr + hlead, hdrs + hfirst, htotal));
    }
    if (total) B2H_OK(sg.in(o_txt + lead, src + first, total));
    B2H_OK(sg.in(o_iv, ivs, n * 16));
    if (unwrap) B2H_OK(sg.in(o_tag, tags, n * 8));
    B2H_OK(sg.in(o_ord, ord.data(), n * 4));
    // in place on the device: the text is staged once
    B2H_OK(bee2hip_beltAE_ragged_stream(unwrap, mode, key, key_len, sg.at(o_iv), hdr_offsets ? sg.at(o_hdr) : nullptr,
                                        hdr_offsets ? sg.at(o_hoff) : nullptr, sg.at(o_txt), sg.at(o_off), sg.at(o_ord), n,
                                        sg.at(o_txt), sg.at(o_tag), unwrap ? sg.at(o_code) : nullptr, nullptr));
    if (total) B2H_OK(sg.out(dst + first, o_txt + lead, total));
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
