// capi_prg.hip -- bash-prg over ragged batches: prg-hash and prg-ae (STB 34.101.77 annexes A.5, A.6; src/crypto/bash/bash_prg.c).
// Part of the C ABI (capi.hip).  One record = one automaton = one lane of bash_prg_ragged_kernel (bash_prg_kernels.hip).
// bee2's own step functions (Start / Absorb / Encr ...) are NOT exported: one automaton is a serial chain, the batch is the product.

// what bashPrgStart asserts (bash_prg.c:115-119) plus the limits of one squeeze; before any device work
static err_t prg_check(size_t l, size_t d, const octet ann[], size_t ann_len, bool keyed, const octet key[], size_t key_len,
                       size_t out_len, size_t n)
{
    if ((l != 128 && l != 192 && l != 256) || (d != 1 && d != 2)) return ERR_BAD_PARAMS;
    if (ann_len % 4 != 0 || ann_len > 60) return ERR_BAD_INPUT;
    if (keyed && (key_len % 4 != 0 || key_len < l / 8 || key_len > 60 || !key)) return ERR_BAD_INPUT;
    if (!keyed && ann_len && !ann) return ERR_BAD_INPUT;
    if (out_len < 1 || out_len > 64) return ERR_BAD_INPUT;
    if (n > 0xffffffffull) return ERR_BAD_INPUT;
    return ERR_OK;
}

static void prg_args(BashPrgArgs &A, uint32_t mode, size_t l, size_t d, const octet fixed[], size_t fixed_len, size_t own_ann_len,
                     size_t out_len)
{
    memset(&A, 0, sizeof A);
    if (fixed_len) memcpy(A.fixed, fixed, fixed_len);
    A.n_fixed = (uint32_t)(fixed_len / 4);
    A.n_ann = (uint32_t)(own_ann_len / 4);
    const size_t ann_len = mode == BASH_PRG_HASH ? fixed_len : own_ann_len, key_len = mode == BASH_PRG_HASH ? 0 : fixed_len;
    A.head = (uint32_t)(ann_len * 4 + key_len / 4);                                 // bash_prg.c:125
    A.cap = (uint32_t)(l / 4 + d);                                                  // bash_prg.c:131
    A.rate = (uint32_t)(key_len ? 192 - l * (2 + d) / 16 : 192 - d * l / 4);        // bash_prg.c:133
    A.mode = mode;
    A.out_len = (uint32_t)out_len;
}

extern "C" err_t bee2hip_bashPrgHash_ragged_stream(size_t l, size_t d, const octet ann[], size_t ann_len, const void *d_data,
                                                   const void *d_offsets, const void *d_order, size_t n, void *d_out,
                                                   size_t out_len, void *stream)
try {
    err_t code = prg_check(l, d, ann, ann_len, false, nullptr, 0, out_len, n);
    if (code != ERR_OK) return code;
    if (misaligned(d_offsets, 8) || misaligned(d_order, 4)) return ERR_BAD_INPUT;
    if (n && (!d_offsets || !d_out)) return ERR_BAD_INPUT;
    code = ensure_device();
    if (code != ERR_OK) return code;
    BashPrgArgs A;
    prg_args(A, BASH_PRG_HASH, l, d, ann, ann_len, 0, out_len);
    return launch_prg_ragged(A, nullptr, d_data, d_offsets, nullptr, nullptr, d_order, n, nullptr, d_out, nullptr, as_stream(stream));
} B2H_CATCH

extern "C" err_t bee2hip_bashPrgAE_ragged_stream(int unwrap, size_t l, size_t d, const octet key[], size_t key_len,
                                                 const void *d_anns, size_t ann_len, const void *d_hdrs,
                                                 const void *d_hdr_offsets, const void *d_src, const void *d_offsets,
                                                 const void *d_order, size_t n, void *d_dst, void *d_tags, size_t tag_len,
                                                 void *d_codes, void *stream)
try {
    err_t code = prg_check(l, d, nullptr, ann_len, true, key, key_len, tag_len, n);
    if (code != ERR_OK) return code;
    if (unwrap != 0 && unwrap != 1) return ERR_BAD_INPUT;
    if (misaligned(d_offsets, 8) || misaligned(d_hdr_offsets, 8) || misaligned(d_order, 4) || misaligned(d_anns, 4) ||
        misaligned(d_codes, 4))
        return ERR_BAD_INPUT;
    if (d_hdrs && !d_hdr_offsets) return ERR_BAD_INPUT;
    if ((d_src == nullptr) != (d_dst == nullptr)) return ERR_BAD_INPUT;
    if (n && (!d_offsets || !d_tags || (ann_len && !d_anns) || (unwrap && !d_codes))) return ERR_BAD_INPUT;
    code = ensure_device();
    if (code != ERR_OK) return code;
    BashPrgArgs A;
    prg_args(A, unwrap ? BASH_PRG_UNWRAP : BASH_PRG_WRAP, l, d, key, key_len, ann_len, tag_len);
    return launch_prg_ragged(A, d_anns, d_hdrs, d_hdr_offsets, d_src, d_offsets, d_order, n, d_dst, d_tags, d_codes,
                             as_stream(stream));
} B2H_CATCH

// ---- host-pointer entries: stage through t_scr[3] (staging.hpp: the ragged part of a Stage), longest record first, one call of
// the stream entry on the NULL stream.  As hash_ragged_host without its host threads: a record's text has to come back from
// wherever it was processed, so nothing is gained by keeping long ones here.
extern "C" err_t bee2hip_bashPrgHash_ragged(size_t l, size_t d, const octet ann[], size_t ann_len, const octet *data,
                                            const uint64_t *offsets, size_t n, octet *out, size_t out_len)
try {
    err_t code = prg_check(l, d, ann, ann_len, false, nullptr, 0, out_len, n);
    if (code != ERR_OK) return code;
    if (n == 0) return ERR_OK;
    if (!offsets || !out || !offsets_rise(offsets, n)) return ERR_BAD_INPUT;
    Stage sg(3, false, "bee2hip_bashPrgHash_ragged staging");
    RaggedPart msg(sg, offsets, n);
    if (msg.total && !data) return ERR_BAD_INPUT;
    std::vector<uint32_t> ord;
    longest_first(ord, offsets, n);
    msg.add_offs(sg);
    const size_t o_ord = sg.add(n * 4), o_out = sg.add(n * out_len);
    B2H_OK(sg.open(16));
    B2H_OK(msg.in(sg, data));
    B2H_OK(sg.in(o_ord, ord.data(), n * 4));
    B2H_OK(bee2hip_bashPrgHash_ragged_stream(l, d, ann, ann_len, msg.data(sg), msg.offs(sg), sg.at(o_ord), n, sg.at(o_out), out_len,
                                             nullptr));
    return sg.out(out, o_out, n * out_len);
} B2H_CATCH

static err_t prg_ae_host(int unwrap, size_t l, size_t d, const octet key[], size_t key_len, const octet *anns, size_t ann_len,
                         const octet *hdrs, const uint64_t *hdr_offsets, const octet *src, const uint64_t *offsets, size_t n,
                         octet *dst, octet *tags, size_t tag_len, err_t *codes)
{
    err_t code = prg_check(l, d, nullptr, ann_len, true, key, key_len, tag_len, n);
    if (code != ERR_OK) return code;
    if (n == 0) return ERR_OK;
    if (!offsets || !tags || (ann_len && !anns) || (unwrap && !codes) || (hdrs && !hdr_offsets)) return ERR_BAD_INPUT;
    if (!offsets_rise(offsets, n) || (hdr_offsets && !offsets_rise(hdr_offsets, n))) return ERR_BAD_INPUT;
    Stage sg(3, false, "bee2hip_bashPrgAE staging");
    RaggedPart txt(sg, offsets, n), hdr(sg, hdr_offsets, n);
    if ((txt.total && (!src || !dst)) || (hdr.total && !hdrs)) return ERR_BAD_INPUT;
    std::vector<uint32_t> ord;
    longest_first(ord, offsets, n);
    const size_t o_ann = sg.add(n * ann_len);
    txt.add_offs(sg);
    hdr.add_offs(sg);
    const size_t o_ord = sg.add(n * 4), o_tag = sg.add(n * tag_len), o_code = sg.add(n * 4);
    B2H_OK(sg.open(16));
    B2H_OK(txt.in(sg, src));
    B2H_OK(hdr.in(sg, hdrs));
    B2H_OK(sg.in(o_ann, anns, n * ann_len));
    if (unwrap) B2H_OK(sg.in(o_tag, tags, n * tag_len));
    B2H_OK(sg.in(o_ord, ord.data(), n * 4));
    // in place on the device: the text is staged once
    B2H_OK(bee2hip_bashPrgAE_ragged_stream(unwrap, l, d, key, key_len, sg.at(o_ann), ann_len, hdr.data(sg), hdr.offs(sg), txt.data(sg),
                                           txt.offs(sg), sg.at(o_ord), n, txt.data(sg), sg.at(o_tag), tag_len,
                                           unwrap ? sg.at(o_code) : nullptr, nullptr));
    B2H_OK(txt.out(sg, dst));
    return unwrap ? sg.out(codes, o_code, n * 4) : sg.out(tags, o_tag, n * tag_len);
}

extern "C" err_t bee2hip_bashPrgAE_wrap_ragged(size_t l, size_t d, const octet key[], size_t key_len, const octet *anns,
                                               size_t ann_len, const octet *hdrs, const uint64_t *hdr_offsets, const octet *src,
                                               const uint64_t *offsets, size_t n, octet *dst, octet *tags, size_t tag_len)
try {
    return prg_ae_host(0, l, d, key, key_len, anns, ann_len, hdrs, hdr_offsets, src, offsets, n, dst, tags, tag_len, nullptr);
} B2H_CATCH

extern "C" err_t bee2hip_bashPrgAE_unwrap_ragged(size_t l, size_t d, const octet key[], size_t key_len, const octet *anns,
                                                 size_t ann_len, const octet *hdrs, const uint64_t *hdr_offsets, const octet *src,
                                                 const uint64_t *offsets, size_t n, const octet *tags, size_t tag_len, octet *dst,
                                                 err_t *codes)
try {
    return prg_ae_host(1, l, d, key, key_len, anns, ann_len, hdrs, hdr_offsets, src, offsets, n, dst, const_cast<octet *>(tags),
                       tag_len, codes);
} B2H_CATCH
