// capi_bpki.hip -- the password-protected containers of STB 34.101.78 (src/crypto/bpki.c:206-548: bpkiPrivkeyWrap / Unwrap,
// bpkiShareWrap / Unwrap) as batches: n containers opened or sealed in one call.  Part of the C ABI (capi.hip), after
// capi_hmac.hip.  A container is beltPBKDF2(pwd, iter, salt) -> beltKWPWrap / Unwrap(.., header = 0, KEK, 32) inside a fixed DER
// frame: the frames are parsed and built on the host (bpki_der.hpp), the passwords are stretched by belt_hmac_batch_kernel, and the
// derived keys go from there to belt_kwp_batch_kernel as its per-record keys without leaving the device.  bee2's own bpki* names
// are NOT exported.
#include "bpki_der.hpp"

constexpr int BPKI_KEK_SLOT = 20;               // stream scratch of the derived keys (no launcher uses this slot)
constexpr size_t BPKI_GROUPS_MAX = 8;           // distinct iteration counts, and distinct token lengths, of one unwrap call

// the derived keys on the device: zeroed on the stream that used them on every way out
struct BpkiKek {
    void *p = nullptr;
    size_t bytes = 0;
    err_t get(size_t n)
    {
        B2H_OK(scratch_for_stream(nullptr, BPKI_KEK_SLOT, n * 32, &p));
        bytes = n * 32;
        return ERR_OK;
    }
    octet *at(size_t i) const { return (octet *)p + 32 * i; }
    ~BpkiKek() { if (p) (void)hipMemsetAsync(p, 0, bytes, nullptr); }
};
struct BpkiWiped {                              // a host vector that held secrets
    std::vector<octet> v;
    ~BpkiWiped() { if (!v.empty()) wipe_host(v.data(), v.size()); }
};

static err_t bpki_args(int kind, size_t n) { return (kind != 0 && kind != 1) || n > 0xffffffffull ? ERR_BAD_INPUT : ERR_OK; }

extern "C" err_t bee2hip_bpkiUnwrap_batch(int kind, const octet *epkis, const uint64_t *epki_offsets, const octet *pwds,
                                          const uint64_t *pwd_offsets, size_t n, octet *keys, uint32_t *key_lens, err_t *codes)
try {
    B2H_OK(bpki_args(kind, n));
    if (n == 0) return ERR_OK;
    if (!epki_offsets || !pwd_offsets || !keys || !key_lens || !codes) return ERR_BAD_INPUT;
    if (!offsets_rise(epki_offsets, n) || !offsets_rise(pwd_offsets, n)) return ERR_BAD_INPUT;
    if ((epki_offsets[n] > epki_offsets[0] && !epkis) || (pwd_offsets[n] > pwd_offsets[0] && !pwds)) return ERR_BAD_INPUT;

    // the outer frames, and bee2's codes in bee2's order (bpki.c:392-411) as far as the host can tell
    std::vector<bpki::Epki> info(n);
    std::vector<err_t> code(n);
    std::vector<uint32_t> live;                 // the records that go to the device, by (iter, token length), then index
    for (size_t i = 0; i < n; ++i) {
        const bpki::Epki &e = info[i] = bpki::epki_parse(epkis ? epkis + epki_offsets[i] : nullptr, (size_t)(epki_offsets[i + 1] - epki_offsets[i]));
        code[i] = !e.ok ? ERR_BAD_FORMAT
                  : e.iter == 0 ? ERR_BAD_INPUT                                  // belt_pbkdf.c:32
                  : e.iter > HMAC_ITER_MAX ? ERR_NOT_IMPLEMENTED
                  : e.edata_len < KWP_TOKEN_MIN ? ERR_BAD_INPUT                  // belt_kwp.c:61
                  : e.edata_len > KWP_TOKEN_MAX ? ERR_NOT_IMPLEMENTED : ERR_OK;
        if (code[i] == ERR_OK) live.push_back((uint32_t)i);
    }
    std::stable_sort(live.begin(), live.end(), [&](uint32_t a, uint32_t b) {
        return info[a].iter != info[b].iter ? info[a].iter < info[b].iter : info[a].edata_len < info[b].edata_len;
    });
    {
        std::vector<uint64_t> iters, lens;
        for (uint32_t i : live) {
            if (std::find(iters.begin(), iters.end(), info[i].iter) == iters.end()) iters.push_back(info[i].iter);
            if (std::find(lens.begin(), lens.end(), (uint64_t)info[i].edata_len) == lens.end()) lens.push_back(info[i].edata_len);
        }
        if (iters.size() > BPKI_GROUPS_MAX || lens.size() > BPKI_GROUPS_MAX) return ERR_NOT_IMPLEMENTED;      // nothing written
    }
    memset(keys, 0, n * bpki::KEY_MAX);
    for (size_t i = 0; i < n; ++i) key_lens[i] = 0;
    const size_t m = live.size();
    if (m == 0) {
        for (size_t i = 0; i < n; ++i) codes[i] = code[i];
        return ERR_OK;                                                           // without a device
    }

    // staged in the order of `live`: passwords and recovered frames (one secret range), tokens, salts, offsets, codes
    std::vector<uint64_t> poff(m + 1), toff(m + 1), doff(m + 1);
    poff[0] = toff[0] = doff[0] = 0;
    for (size_t k = 0; k < m; ++k) {
        const uint32_t i = live[k];
        poff[k + 1] = poff[k] + (pwd_offsets[i + 1] - pwd_offsets[i]);
        toff[k + 1] = toff[k] + info[i].edata_len;
        doff[k + 1] = doff[k] + (info[i].edata_len - 16);
    }
    Stage sg(3, false, "bee2hip_bpkiUnwrap_batch staging");
    const size_t o_pwd = sg.add(poff[m]), o_dst = sg.add(doff[m]), o_tok = sg.add(toff[m]), o_salt = sg.add(m * 8),
                 o_poff = sg.add((m + 1) * 8), o_code = sg.add(m * 4);
    sg.secret(o_pwd, o_dst + doff[m] - o_pwd);
    B2H_OK(sg.open(16));
    {
        BpkiWiped pw;
        pw.v.resize(poff[m]);
        std::vector<octet> tok(toff[m]), salt(m * 8);
        for (size_t k = 0; k < m; ++k) {
            const uint32_t i = live[k];
            if (poff[k + 1] > poff[k]) memcpy(pw.v.data() + poff[k], pwds + pwd_offsets[i], poff[k + 1] - poff[k]);
            memcpy(tok.data() + toff[k], epkis + epki_offsets[i] + info[i].edata_off, info[i].edata_len);
            memcpy(salt.data() + 8 * k, info[i].salt, 8);
        }
        B2H_OK(sg.in(o_pwd, pw.v.data(), poff[m]));
        B2H_OK(sg.in(o_tok, tok.data(), toff[m]));
        B2H_OK(sg.in(o_salt, salt.data(), m * 8));
        B2H_OK(sg.in(o_poff, poff.data(), (m + 1) * 8));
    }
    BpkiKek kek;
    B2H_OK(kek.get(m));
    for (size_t g0 = 0, g1; g0 < m; g0 = g1) {                                   // one PBKDF2 launch per iteration count
        for (g1 = g0 + 1; g1 < m && info[live[g1]].iter == info[live[g0]].iter; ++g1) {}
        B2H_OK(bee2hip_beltPBKDF2_batch_stream(sg.at(o_pwd), sg.at(o_poff + 8 * g0), (size_t)info[live[g0]].iter, sg.at(o_salt + 8 * g0), 8,
                                               8, nullptr, g1 - g0, kek.at(g0), nullptr));
    }
    for (size_t g0 = 0, g1; g0 < m; g0 = g1) {                                   // one kwp launch per run of one token length
        const size_t T = info[live[g0]].edata_len;
        for (g1 = g0 + 1; g1 < m && info[live[g1]].edata_len == T; ++g1) {}
        B2H_OK(bee2hip_beltKWP_keyed_batch_stream(1, kek.at(g0), 32, nullptr, sg.at(o_tok + toff[g0]), T, g1 - g0,
                                                  sg.at(o_dst + doff[g0]), sg.at(o_code + 4 * g0), nullptr));
    }
    std::vector<err_t> kcode(m);
    BpkiWiped pki;
    pki.v.resize(doff[m]);
    B2H_OK(sg.out(kcode.data(), o_code, m * 4));
    B2H_OK(sg.out(pki.v.data(), o_dst, doff[m]));
    for (size_t k = 0; k < m; ++k) {                                             // bpki.c:410-424, :530-547
        const uint32_t i = live[k];
        octet *key = keys + bpki::KEY_MAX * i;
        if (kcode[k] != ERR_OK) { code[i] = kcode[k]; continue; }
        const size_t len = bpki::pki_parse(kind, pki.v.data() + doff[k], (size_t)(doff[k + 1] - doff[k]), key);
        if (len == 0) code[i] = ERR_BAD_FORMAT;
        else if (kind == 1 && (key[0] < 1 || key[0] > 16)) {
            code[i] = ERR_BAD_SHAREKEY;
            memset(key, 0, bpki::KEY_MAX);
        } else key_lens[i] = (uint32_t)len;
    }
    for (size_t i = 0; i < n; ++i) codes[i] = code[i];
    return ERR_OK;
} B2H_CATCH

extern "C" err_t bee2hip_bpkiWrap_batch(int kind, const octet *keys, size_t key_len, const octet *pwds, const uint64_t *pwd_offsets,
                                        const octet *salts, size_t iter, size_t n, octet *epkis, size_t *epki_len)
try {
    B2H_OK(bpki_args(kind, n));
    if (iter < 10000) return ERR_BAD_INPUT;                                      // bpki.c:323, :443
    const size_t pki_len = bpki::pki_build(nullptr, kind, nullptr, key_len);
    if (pki_len == 0) return kind ? ERR_BAD_SECKEY : ERR_BAD_PRIVKEY;            // bpki.c:325-327, :445-447
    if (kind == 1 && keys)                                                       // bpki.c:446: before the length, so a length query too
        for (size_t i = 0; i < n; ++i)
            if (keys[key_len * i] < 1 || keys[key_len * i] > 16) return ERR_BAD_SECKEY;
    if (iter > HMAC_ITER_MAX) return ERR_NOT_IMPLEMENTED;
    const size_t T = pki_len + 16, L = bpki::epki_build(nullptr, nullptr, iter, nullptr, T, nullptr);
    if (epki_len) *epki_len = L;
    if (!epkis || n == 0) return ERR_OK;
    if (!keys || !pwd_offsets || !salts || !offsets_rise(pwd_offsets, n)) return ERR_BAD_INPUT;
    const size_t pwd_first = (size_t)pwd_offsets[0], pwd_total = (size_t)(pwd_offsets[n] - pwd_offsets[0]);
    if (pwd_total && !pwds) return ERR_BAD_INPUT;

    Stage sg(3, false, "bee2hip_bpkiWrap_batch staging");
    const size_t o_pwd = sg.add(pwd_total), o_src = sg.add(n * pki_len), o_dst = sg.add(n * T), o_salt = sg.add(n * 8),
                 o_poff = sg.add((n + 1) * 8);
    sg.secret(o_pwd, o_src + n * pki_len - o_pwd);
    B2H_OK(sg.open(16));
    {
        BpkiWiped pki;
        pki.v.resize(n * pki_len);
        std::vector<uint64_t> poff(n + 1);
        for (size_t i = 0; i < n; ++i) bpki::pki_build(pki.v.data() + pki_len * i, kind, keys + key_len * i, key_len);
        for (size_t i = 0; i <= n; ++i) poff[i] = pwd_offsets[i] - pwd_first;
        B2H_OK(sg.in(o_pwd, pwds + pwd_first, pwd_total));
        B2H_OK(sg.in(o_src, pki.v.data(), n * pki_len));
        B2H_OK(sg.in(o_salt, salts, n * 8));
        B2H_OK(sg.in(o_poff, poff.data(), (n + 1) * 8));
    }
    BpkiKek kek;
    B2H_OK(kek.get(n));
    B2H_OK(bee2hip_beltPBKDF2_batch_stream(sg.at(o_pwd), sg.at(o_poff), iter, sg.at(o_salt), 8, 8, nullptr, n, kek.at(0), nullptr));
    B2H_OK(bee2hip_beltKWP_keyed_batch_stream(0, kek.at(0), 32, nullptr, sg.at(o_src), pki_len, n, sg.at(o_dst), nullptr, nullptr));
    std::vector<octet> tok(n * T);
    B2H_OK(sg.out(tok.data(), o_dst, n * T));
    for (size_t i = 0; i < n; ++i) bpki::epki_build(epkis + L * i, salts + 8 * i, iter, tok.data() + T * i, T, nullptr);
    return ERR_OK;
} B2H_CATCH
