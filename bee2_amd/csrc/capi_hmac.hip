// capi_hmac.hip -- belt-hmac and belt-pbkdf2 (STB 34.101.31; src/crypto/belt/belt_hmac.c, belt_pbkdf.c): n MACs written or
// checked, n passwords stretched into n keys, and bee2's two one-shots.  Part of the C ABI (capi.hip), after capi_kwp.hip.  One
// record = one lane of belt_hmac_batch_kernel (belt_hmac_kernels.hip); a single record on the host is host_hmac.hpp.  bee2's
// step functions beltHMAC_keep / Start / StepA / StepG* / StepV* are NOT exported.
#include "host_hmac.hpp"

// what the HMAC entries refuse before any device work; given = the per-record key form is there
static err_t belthmac_check(int verify, const octet key[], bool given, size_t mac_len, size_t n)
{
    if (verify != 0 && verify != 1) return ERR_BAD_INPUT;
    if (mac_len < 1 || mac_len > 32) return ERR_BAD_INPUT;
    if (n > 0xffffffffull) return ERR_BAD_INPUT;
    if (key && given) return ERR_BAD_INPUT;                              // both key forms
    if (n && !key && !given) return ERR_BAD_INPUT;                       // neither
    return ERR_OK;
}
static err_t beltpbkdf2_check(size_t iter, size_t salt_len, size_t salt_stride, size_t n)
{
    if (iter == 0) return ERR_BAD_INPUT;                                 // belt_pbkdf.c:32
    if (n > 0xffffffffull) return ERR_BAD_INPUT;
    if (salt_stride != 0 && salt_stride < salt_len) return ERR_BAD_INPUT;
    if (iter > HMAC_ITER_MAX) return ERR_NOT_IMPLEMENTED;
    return ERR_OK;
}

extern "C" err_t bee2hip_beltHMAC_ragged_stream(int verify, const octet key[], size_t key_len, const void *d_keys,
                                                const void *d_key_offsets, const void *d_data, const void *d_offsets,
                                                const void *d_order, size_t n, void *d_macs, size_t mac_len, void *d_codes,
                                                void *stream)
try {
    err_t code = belthmac_check(verify, key, d_keys || d_key_offsets, mac_len, n);
    if (code != ERR_OK) return code;
    if (misaligned(d_offsets, 8) || misaligned(d_key_offsets, 8) || misaligned(d_order, 4) || misaligned(d_codes, 4))
        return ERR_BAD_INPUT;
    if (n && (!d_offsets || !d_macs || (verify && !d_codes) || (!key && !d_key_offsets))) return ERR_BAD_INPUT;
    if (n == 0) return ERR_OK;
    code = ensure_device();
    if (code != ERR_OK) return code;
    HmacArgs A;
    memset(&A, 0, sizeof A);
    if (key) {
        hostp::hmac_key_state(hostT(), host_beltH(), key, key_len, A.ks);
        A.shared = 1;
    }
    A.iter = 1;
    A.mac_len = (uint32_t)mac_len;
    A.verify = (uint32_t)verify;
    code = launch_belt_hmac_batch(A, d_keys, d_key_offsets, d_data, d_offsets, d_order, n, d_macs, d_codes, as_stream(stream));
    wipe_host(&A, sizeof A);
    return code;
} B2H_CATCH

extern "C" err_t bee2hip_beltPBKDF2_batch_stream(const void *d_pwds, const void *d_pwd_offsets, size_t iter, const void *d_salts,
                                                 size_t salt_len, size_t salt_stride, const void *d_order, size_t n, void *d_keys,
                                                 void *stream)
try {
    err_t code = beltpbkdf2_check(iter, salt_len, salt_stride, n);
    if (code != ERR_OK) return code;
    if (misaligned(d_pwd_offsets, 8) || misaligned(d_order, 4)) return ERR_BAD_INPUT;
    if (n && (!d_pwd_offsets || !d_keys || (salt_len && !d_salts))) return ERR_BAD_INPUT;
    if (n == 0) return ERR_OK;
    code = ensure_device();
    if (code != ERR_OK) return code;
    HmacArgs A;
    memset(&A, 0, sizeof A);
    A.suffix = 4;
    A.iter = (uint32_t)iter;
    A.mac_len = 32;
    A.msg_len = salt_len;
    A.msg_stride = salt_stride;
    return launch_belt_hmac_batch(A, d_pwds, d_pwd_offsets, d_salts, nullptr, d_order, n, d_keys, nullptr, as_stream(stream));
} B2H_CATCH

// ---- host-pointer entries, as beltae_host: one Stage with its ragged parts (staging.hpp), longest record first, one call of
// the stream entry on the NULL stream.  The keys are marked secret: their staging is zeroed when the Stage goes.
static err_t belthmac_host(int verify, const octet key[], size_t key_len, const octet *keys, const uint64_t *key_offsets,
                           const octet *data, const uint64_t *offsets, size_t n, octet *macs, size_t mac_len, err_t *codes)
{
    const err_t code = belthmac_check(verify, key, keys || key_offsets, mac_len, n);
    if (code != ERR_OK) return code;
    if (n == 0) return ERR_OK;
    if (!offsets || !macs || (verify && !codes) || (!key && !key_offsets)) return ERR_BAD_INPUT;
    if (!offsets_rise(offsets, n) || (key_offsets && !offsets_rise(key_offsets, n))) return ERR_BAD_INPUT;
    Stage sg(3, false, "bee2hip_beltHMAC staging");
    RaggedPart msg(sg, offsets, n), kys(sg, key_offsets, n);
    if ((msg.total && !data) || (kys.total && !keys)) return ERR_BAD_INPUT;
    std::vector<uint32_t> ord;
    longest_first(ord, offsets, n);
    msg.add_offs(sg);
    kys.add_offs(sg);
    const size_t o_ord = sg.add(n * 4), o_mac = sg.add(n * mac_len), o_code = sg.add(n * 4);
    sg.secret(kys.o_data, kys.lead + kys.total);
    B2H_OK(sg.open(16));
    B2H_OK(msg.in(sg, data));
    B2H_OK(kys.in(sg, keys));
    if (verify) B2H_OK(sg.in(o_mac, macs, n * mac_len));
    B2H_OK(sg.in(o_ord, ord.data(), n * 4));
    B2H_OK(bee2hip_beltHMAC_ragged_stream(verify, key, key_len, kys.data(sg), kys.offs(sg), msg.data(sg), msg.offs(sg), sg.at(o_ord), n,
                                          sg.at(o_mac), mac_len, verify ? sg.at(o_code) : nullptr, nullptr));
    return verify ? sg.out(codes, o_code, n * 4) : sg.out(macs, o_mac, n * mac_len);
}

extern "C" err_t bee2hip_beltHMAC_ragged(const octet key[], size_t key_len, const octet *keys, const uint64_t *key_offsets,
                                         const octet *data, const uint64_t *offsets, size_t n, octet *macs, size_t mac_len)
try {
    return belthmac_host(0, key, key_len, keys, key_offsets, data, offsets, n, macs, mac_len, nullptr);
} B2H_CATCH

extern "C" err_t bee2hip_beltHMAC_verify_ragged(const octet key[], size_t key_len, const octet *keys, const uint64_t *key_offsets,
                                                const octet *data, const uint64_t *offsets, size_t n, const octet *macs,
                                                size_t mac_len, err_t *codes)
try {
    return belthmac_host(1, key, key_len, keys, key_offsets, data, offsets, n, const_cast<octet *>(macs), mac_len, codes);
} B2H_CATCH

// the passwords and, next to them, the derived keys are the secret range; longest password first (the salts have one length)
static err_t beltpbkdf2_host(const octet *pwds, const uint64_t *pwd_offsets, size_t iter, const octet *salts, size_t salt_len,
                             size_t salt_stride, size_t n, octet *keys)
{
    const err_t code = beltpbkdf2_check(iter, salt_len, salt_stride, n);
    if (code != ERR_OK) return code;
    if (n == 0) return ERR_OK;
    if (!pwd_offsets || !keys || (salt_len && !salts)) return ERR_BAD_INPUT;
    if (!offsets_rise(pwd_offsets, n)) return ERR_BAD_INPUT;
    Stage sg(3, false, "bee2hip_beltPBKDF2 staging");
    RaggedPart pwd(sg, pwd_offsets, n);
    if (pwd.total && !pwds) return ERR_BAD_INPUT;
    std::vector<uint32_t> ord;
    longest_first(ord, pwd_offsets, n);
    const size_t salt_bytes = (n - 1) * salt_stride + salt_len;
    const size_t o_key = sg.add(n * 32), o_salt = sg.add(salt_bytes);        // (the keys right behind the passwords: one secret range)
    pwd.add_offs(sg);
    const size_t o_ord = sg.add(n * 4);
    sg.secret(pwd.o_data, o_key + n * 32 - pwd.o_data);
    B2H_OK(sg.open(16));
    B2H_OK(pwd.in(sg, pwds));
    B2H_OK(sg.in(o_salt, salts, salt_bytes));
    B2H_OK(sg.in(o_ord, ord.data(), n * 4));
    B2H_OK(bee2hip_beltPBKDF2_batch_stream(pwd.data(sg), pwd.offs(sg), iter, sg.at(o_salt), salt_len, salt_stride, sg.at(o_ord), n,
                                           sg.at(o_key), nullptr));
    return sg.out(keys, o_key, n * 32);
}

extern "C" err_t bee2hip_beltPBKDF2_batch(const octet *pwds, const uint64_t *pwd_offsets, size_t iter, const octet *salts,
                                          size_t salt_len, size_t salt_stride, size_t n, octet *keys)
try {
    return beltpbkdf2_host(pwds, pwd_offsets, iter, salts, salt_len, salt_stride, n, keys);
} B2H_CATCH

// ---- bee2's one-shots (belt_hmac.c:244-263, belt_pbkdf.c:24-65): one record is one serial chain, so the host runs it unless the
// path policy sends every call to the GPU; then it is a batch of one
extern "C" err_t beltHMAC(octet mac[32], const void *src, size_t count, const octet key[], size_t len)
try {
    if ((count && !src) || (len && !key) || !mac) return ERR_BAD_INPUT;
    return with_host(K_SERIAL, count, "beltHMAC", [&]() -> err_t {
        const uint64_t koff[2] = {0, len}, off[2] = {0, count};
        octet out[32];
        B2H_OK(belthmac_host(0, nullptr, 0, key, koff, (const octet *)src, off, 1, out, 32, nullptr));
        memcpy(mac, out, 32);
        return ERR_OK;
    }, [&] {
        HmacKeyState ks;
        octet out[32];                                               // (mac may be part of src)
        hostp::hmac_run(hostT(), host_beltH(), ks, 0, key, len, (const octet *)src, count, 0, 1, out);
        memcpy(mac, out, 32);
        wipe_host(&ks, sizeof ks);
    });
} B2H_CATCH

extern "C" err_t beltPBKDF2(octet key[32], const octet pwd[], size_t pwd_len, size_t iter, const octet salt[], size_t salt_len)
try {
    if (iter == 0 || (pwd_len && !pwd) || (salt_len && !salt) || !key) return ERR_BAD_INPUT;
    const auto host = [&] {
        HmacKeyState ks;
        octet out[32];                                               // (bee2's own test derives a key over its salt)
        hostp::hmac_run(hostT(), host_beltH(), ks, 0, pwd, pwd_len, salt, salt_len, 4, iter, out);
        memcpy(key, out, 32);
        wipe_host(&ks, sizeof ks);
        wipe_host(out, sizeof out);
    };
    if (iter > HMAC_ITER_MAX) {                                      // above the cap of one launch: the host, whatever the policy
        B2H_OK(device_seen());
        host();
        g_n_host.fetch_add(1, std::memory_order_relaxed);
        return ERR_OK;
    }
    return with_host(K_SERIAL, 4 * iter * 32, "beltPBKDF2", [&]() -> err_t {
        const uint64_t poff[2] = {0, pwd_len};
        octet out[32];
        B2H_OK(beltpbkdf2_host(pwd, poff, iter, salt, salt_len, 0, 1, out));
        memcpy(key, out, 32);
        wipe_host(out, sizeof out);
        return ERR_OK;
    }, host);
} B2H_CATCH
