// capi_kwp.hip -- belt-kwp, the key wrap of STB 34.101.31 (src/crypto/belt/belt_kwp.c), as a batch: n keys of one length under
// one key-encryption key or (the _keyed_ entries) under one key-encryption key each, each with its own header.  Part of the C
// ABI (capi.hip), after capi_fmt.hip.  One record = one lane of belt_kwp_batch_kernel (belt_kwp_kernels.hip).  bee2's one-shots beltKWPWrap / beltKWPUnwrap are NOT exported: a single
// token is one serial chain.

// what the batch entries refuse before any device work; count = the octets of a record of src
static err_t beltkwp_check(int unwrap, const octet key[], size_t key_len, size_t count, size_t n)
{
    if (unwrap != 0 && unwrap != 1) return ERR_BAD_INPUT;
    if (count < (unwrap ? 32u : 16u)) return ERR_BAD_INPUT;              // belt_kwp.c:29, :61
    if (!key_len_ok(key_len) || !key) return ERR_BAD_INPUT;
    if (n > 0xffffffffull) return ERR_BAD_INPUT;
    if (count + (unwrap ? 0u : 16u) > KWP_TOKEN_MAX) return ERR_NOT_IMPLEMENTED;
    return ERR_OK;
}
// two ranges that share an octet
static inline bool kwp_ranges_meet(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

extern "C" err_t bee2hip_beltKWP_batch_stream(int unwrap, const octet key[], size_t key_len, const void *d_hdrs, const void *d_src,
                                              size_t count, size_t n, void *d_dst, void *d_codes, void *stream)
try {
    err_t code = beltkwp_check(unwrap, key, key_len, count, n);
    if (code != ERR_OK) return code;
    if (n && (!d_src || !d_dst || (unwrap && !d_codes))) return ERR_BAD_INPUT;
    if (unwrap && misaligned(d_codes, 4)) return ERR_BAD_INPUT;
    if (n == 0) return ERR_OK;
    if (kwp_ranges_meet(d_src, n * count, d_dst, n * (unwrap ? count - 16 : count + 16))) return ERR_BAD_INPUT;
    code = ensure_device();
    if (code != ERR_OK) return code;
    u32 kw[8];
    beltKeyExpand2(kw, key, key_len);
    code = launch_belt_kwp_batch(unwrap, count, kw, nullptr, 0, d_hdrs, d_src, n, d_dst, d_codes, as_stream(stream));
    wipe_host(kw, sizeof kw);
    return code;
} B2H_CATCH

// one Stage: the records, the results, the headers and the codes side by side (source and result differ in size, so the
// device never works in place; the caller's dst may be its src)
static err_t beltkwp_host(int unwrap, const octet key[], size_t key_len, const octet *hdrs, const octet *src, size_t count, size_t n,
                          octet *dst, err_t *codes)
{
    const err_t code = beltkwp_check(unwrap, key, key_len, count, n);
    if (code != ERR_OK) return code;
    if (n && (!src || !dst || (unwrap && !codes))) return ERR_BAD_INPUT;
    if (n == 0) return ERR_OK;
    const size_t in_bytes = n * count, out_bytes = n * (unwrap ? count - 16 : count + 16);
    Stage sg(3, false, "bee2hip_beltKWP staging");
    const size_t o_src = sg.add(in_bytes), o_dst = sg.add(out_bytes), o_hdr = sg.add(hdrs ? n * 16 : 0),
                 o_codes = sg.add(unwrap ? n * sizeof(err_t) : 0);
    sg.secret(unwrap ? o_dst : o_src, unwrap ? out_bytes : in_bytes);    // the keys in the clear
    B2H_OK(sg.open());
    B2H_OK(sg.in(o_src, src, in_bytes));
    if (hdrs) B2H_OK(sg.in(o_hdr, hdrs, n * 16));
    B2H_OK(bee2hip_beltKWP_batch_stream(unwrap, key, key_len, hdrs ? sg.at(o_hdr) : nullptr, sg.at(o_src), count, n, sg.at(o_dst),
                                        unwrap ? sg.at(o_codes) : nullptr, nullptr));
    if (unwrap) B2H_OK(sg.out(codes, o_codes, n * sizeof(err_t)));
    return sg.out(dst, o_dst, out_bytes);
}

extern "C" err_t bee2hip_beltKWP_wrap_batch(const octet key[], size_t key_len, const octet *hdrs, const octet *src, size_t count,
                                            size_t n, octet *dst)
try {
    return beltkwp_host(0, key, key_len, hdrs, src, count, n, dst, nullptr);
} B2H_CATCH

extern "C" err_t bee2hip_beltKWP_unwrap_batch(const octet key[], size_t key_len, const octet *hdrs, const octet *src, size_t count,
                                              size_t n, octet *dst, err_t *codes)
try {
    return beltkwp_host(1, key, key_len, hdrs, src, count, n, dst, codes);
} B2H_CATCH

// ---- one key-encryption key per record: record i is beltKWPWrap / beltKWPUnwrap(dst_i, src_i, count, hdr_i, keys + i * key_len, key_len)
static err_t beltkwp_keyed_check(int unwrap, size_t key_len, size_t count, size_t n)
{
    if (unwrap != 0 && unwrap != 1) return ERR_BAD_INPUT;
    if (count < (unwrap ? 32u : 16u)) return ERR_BAD_INPUT;              // belt_kwp.c:29, :61
    if (!key_len_ok(key_len)) return ERR_BAD_INPUT;
    if (n > 0xffffffffull) return ERR_BAD_INPUT;
    if (count + (unwrap ? 0u : 16u) > KWP_TOKEN_MAX) return ERR_NOT_IMPLEMENTED;
    return ERR_OK;
}

extern "C" err_t bee2hip_beltKWP_keyed_batch_stream(int unwrap, const void *d_keys, size_t key_len, const void *d_hdrs,
                                                    const void *d_src, size_t count, size_t n, void *d_dst, void *d_codes, void *stream)
try {
    err_t code = beltkwp_keyed_check(unwrap, key_len, count, n);
    if (code != ERR_OK) return code;
    if (n && (!d_keys || !d_src || !d_dst || (unwrap && !d_codes))) return ERR_BAD_INPUT;
    if (unwrap && misaligned(d_codes, 4)) return ERR_BAD_INPUT;
    if (n == 0) return ERR_OK;
    const size_t out_bytes = n * (unwrap ? count - 16 : count + 16);
    if (kwp_ranges_meet(d_src, n * count, d_dst, out_bytes) || kwp_ranges_meet(d_keys, n * key_len, d_dst, out_bytes)) return ERR_BAD_INPUT;
    code = ensure_device();
    if (code != ERR_OK) return code;
    return launch_belt_kwp_batch(unwrap, count, nullptr, d_keys, key_len, d_hdrs, d_src, n, d_dst, d_codes, as_stream(stream));
} B2H_CATCH

// one Stage as beltkwp_host; the key-encryption keys sit next to the keys in the clear (wrap: in front of src, unwrap: behind
// dst), so that one secret range covers both
static err_t beltkwp_keyed_host(int unwrap, const octet *keys, size_t key_len, const octet *hdrs, const octet *src, size_t count,
                                size_t n, octet *dst, err_t *codes)
{
    const err_t code = beltkwp_keyed_check(unwrap, key_len, count, n);
    if (code != ERR_OK) return code;
    if (n && (!keys || !src || !dst || (unwrap && !codes))) return ERR_BAD_INPUT;
    if (n == 0) return ERR_OK;
    const size_t in_bytes = n * count, out_bytes = n * (unwrap ? count - 16 : count + 16), key_bytes = n * key_len;
    Stage sg(3, false, "bee2hip_beltKWP keyed staging");
    size_t o_key, o_src, o_dst;
    if (unwrap) {
        o_src = sg.add(in_bytes), o_dst = sg.add(out_bytes), o_key = sg.add(key_bytes);
        sg.secret(o_dst, o_key + key_bytes - o_dst);
    } else {
        o_key = sg.add(key_bytes), o_src = sg.add(in_bytes), o_dst = sg.add(out_bytes);
        sg.secret(o_key, o_src + in_bytes - o_key);
    }
    const size_t o_hdr = sg.add(hdrs ? n * 16 : 0), o_codes = sg.add(unwrap ? n * sizeof(err_t) : 0);
    B2H_OK(sg.open());
    B2H_OK(sg.in(o_key, keys, key_bytes));
    B2H_OK(sg.in(o_src, src, in_bytes));
    if (hdrs) B2H_OK(sg.in(o_hdr, hdrs, n * 16));
    B2H_OK(bee2hip_beltKWP_keyed_batch_stream(unwrap, sg.at(o_key), key_len, hdrs ? sg.at(o_hdr) : nullptr, sg.at(o_src), count, n,
                                              sg.at(o_dst), unwrap ? sg.at(o_codes) : nullptr, nullptr));
    if (unwrap) B2H_OK(sg.out(codes, o_codes, n * sizeof(err_t)));
    return sg.out(dst, o_dst, out_bytes);
}

extern "C" err_t bee2hip_beltKWP_wrap_keyed_batch(const octet *keys, size_t key_len, const octet *hdrs, const octet *src, size_t count,
                                                  size_t n, octet *dst)
try {
    return beltkwp_keyed_host(0, keys, key_len, hdrs, src, count, n, dst, nullptr);
} B2H_CATCH

extern "C" err_t bee2hip_beltKWP_unwrap_keyed_batch(const octet *keys, size_t key_len, const octet *hdrs, const octet *src,
                                                    size_t count, size_t n, octet *dst, err_t *codes)
try {
    return beltkwp_keyed_host(1, keys, key_len, hdrs, src, count, n, dst, codes);
} B2H_CATCH
