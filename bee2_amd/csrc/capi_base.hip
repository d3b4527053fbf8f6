// capi_base.hip -- management entry points, the device- and host-pointer batch entries of the primitives (bashF, belt block,
// CTR blocks) and the helpers every drop-in file uses (encr_host_blocks, die_on).  Part of the C ABI (capi.hip).
// ============================================================== management ===
extern "C" err_t bee2hip_set_device(int device)
try {
    B2H_TRY(hipSetDevice(device));
    return ensure_device();
} B2H_CATCH
extern "C" err_t bee2hip_sync(void *stream)
try {
    B2H_TRY(hipStreamSynchronize(as_stream(stream)));
    return ERR_OK;
} B2H_CATCH
extern "C" const char *bee2hip_last_error(void) { return t_err; }
extern "C" const char *bee2hip_version(void) { return "bee2hip 0.1 gfx950"; }

// ===================================================== device-pointer batch ===
extern "C" err_t bee2hip_bashF_batch_dev(void *d_states, size_t n, void *stream)
try {
    if (misaligned(d_states, 16)) return ERR_BAD_INPUT;
    if (n && !d_states) return ERR_BAD_INPUT;
    return launch_bashF_batch(d_states, n, as_stream(stream));
} B2H_CATCH

extern "C" err_t bee2hip_beltCTR_blocks_dev(void *d_buf, size_t nblocks, const u32 key[8],
                                            const u32 ctr0[4], uint64_t first_block, void *stream)
try {
    if (misaligned(d_buf, 16)) return ERR_BAD_INPUT;
    if ((nblocks && !d_buf) || !key || !ctr0) return ERR_BAD_INPUT;
    err_t code = ensure_device();
    if (code != ERR_OK) return code;
    return launch_belt_ctr_blocks(d_buf, nblocks, key, ctr0, first_block, nullptr, as_stream(stream));
} B2H_CATCH

extern "C" err_t bee2hip_beltBlockEncr_dev(void *d_blocks, size_t nblocks, const u32 key[8], void *stream)
try {
    if (misaligned(d_blocks, 16)) return ERR_BAD_INPUT;
    if ((nblocks && !d_blocks) || !key) return ERR_BAD_INPUT;
    err_t code = ensure_device();
    if (code != ERR_OK) return code;
    return launch_belt_encr_blocks(d_blocks, nblocks, key, as_stream(stream));
} B2H_CATCH

// ======================================================= host-pointer batch ===
extern "C" err_t bee2hip_bashF_batch(octet *states, size_t n)
try {
    if (n == 0) return ERR_OK;
    if (!states) return ERR_BAD_INPUT;
    Stage sg(0, false, "bee2hip_bashF_batch staging");
    const size_t o = sg.add(n * 192);
    B2H_OK(sg.open());
    if (n * 192 >= DUPLEX_MIN)              // chunks of 2^16 states = 12 MiB: upload, permute and download overlap
        return duplex_inplace(states, sg.at(o), 192, n, (size_t)1 << DUPLEX_LOG2_STATES,
                              [](octet *d, size_t, size_t cnt, hipStream_t st) { return launch_bashF_batch(d, cnt, st); });
    B2H_OK(sg.in(o, states, n * 192));
    B2H_OK(launch_bashF_batch(sg.at(o), n, nullptr));
    return sg.out(states, o, n * 192);
} B2H_CATCH

// E_K over host blocks (n small): the only way the drop-in layer evaluates belt
static err_t encr_host_blocks(uint32_t *blocks, size_t n, const u32 key[8])
{
    return with_host(K_PRIM, n * 16, "belt block encryption", [&]() -> err_t {
        Stage sg(1, false, "belt block encryption staging");
        const size_t o = sg.add(n * 16);
        B2H_OK(sg.open());
        B2H_OK(sg.in(o, blocks, n * 16));
        B2H_OK(launch_belt_encr_blocks(sg.at(o), n, key, nullptr));
        return sg.out(blocks, o, n * 16);
    }, [&] { for (size_t i = 0; i < n; ++i) hostp::belt_encr(hostT(), blocks + 4 * i, key); });
}

// the belt key lengths (belt.h)
static inline bool key_len_ok(size_t len) { return len == 16 || len == 24 || len == 32; }

// a device failure inside a void bee2 function cannot be reported through the bee2
// signature: fail loudly instead of returning wrong bytes.
static void die_on(err_t code, const char *where)
{
    if (code == ERR_OK) return;
    fprintf(stderr, "libbee2hip: %s failed (err %u): %s\n", where, (unsigned)code, t_err);
    abort();
}

