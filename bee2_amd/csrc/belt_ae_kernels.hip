// belt_ae_kernels.hip -- belt-dwp and belt-che (STB 34.101.31, src/crypto/belt/belt_dwp.c, belt_che.c) over a ragged batch of
// records, one record per lane.  Device side of bee2hip_beltAE_*_ragged* (capi_beltae.hip).  Part of bee2hip_tu_belt.hip, after
// belt_kernels.hip (BeltKey, ctr_at) and mixed_kernels.hip (the ragged launch order).
#pragma once
#include "belt_dev.hpp"
#include "common.hpp"

namespace bee2hip {

// what a launch is told by value (the key never sits in device memory the library does not own)
struct BeltAeArgs {
    BeltKey key;
    uint32_t t0[4];         // beltH()[0..16): the start value of t
    uint32_t mode;          // 0 belt-dwp, 1 belt-che
    uint32_t unwrap;
};

constexpr int AE_WG = 256;                              // four wavefronts
typedef BeltTabSmall AeTab;                             // 4 KiB: two workgroups per CU beside the multiplier tables
constexpr int AE_GF_BYTES = 16 * 64 * 16;               // per wavefront: 16 multiples of r, one 16-octet entry per lane
constexpr int AE_LDS = AeTab::kBytes + (AE_WG / 64) * AE_GF_BYTES;

// t * r with a multiplier of the lane's own: the 16 products v(x) * r, deg v < 4, in LDS as [entry][lane] -- entry v of lane l
// is uint4 number 64 v + l of the wavefront's 16 KiB, so its banks are 4 l .. 4 l + 3 (mod 64) whatever v is: the 16 lanes
// that ds_read_b128 serves together never meet in a bank, and which entry a lane reads shows in no LDS cycle.  Horner over the
// 32 nibbles of t, most significant first: acc <- acc x^4 ^ T[nibble].
struct GfLaneTab {
    uint4 *t;               // entry 0 of this lane
    __device__ explicit GfLaneTab(uint8_t *gf) : t(reinterpret_cast<uint4 *>(gf) + (threadIdx.x >> 6) * (AE_GF_BYTES / 16) + (threadIdx.x & 63)) {}
    __device__ __forceinline__ void build(const Gf128 r) const
    {
        Gf128 m[4];
        m[0] = r;
#pragma unroll
        for (int k = 1; k < 4; ++k) m[k] = gf_mul_xk(m[k - 1], 1);
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            Gf128 e = {0, 0};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((v >> k) & 1) { e.lo ^= m[k].lo; e.hi ^= m[k].hi; }
            t[64 * v] = gf_to(e);
        }
    }
    __device__ __forceinline__ Gf128 mul(const Gf128 a) const
    {
        const uint32_t w[4] = {(uint32_t)a.lo, (uint32_t)(a.lo >> 32), (uint32_t)a.hi, (uint32_t)(a.hi >> 32)};
        Gf128 acc = {0, 0};
#pragma unroll
        for (int p = 31; p >= 0; --p) {
            const uint32_t v = (w[p >> 3] >> (4 * (p & 7))) & 15u;
            const uint4 e = t[64 * v];
            if (p != 31) acc = gf_mul_xk(acc, 4);
            acc.lo ^= (uint64_t)e.x | (uint64_t)e.y << 32;
            acc.hi ^= (uint64_t)e.z | (uint64_t)e.w << 32;
        }
        return acc;
    }
};

// the first cnt <= 16 octets at p (any alignment) as four little-endian words, zeros behind: the one or two aligned quads that
// hold them, shifted by p mod 16 (bash_ragged_kernel); a quad without an octet of the block is not read
__device__ __forceinline__ void ae_load(uint32_t (&x)[4], const uint8_t *p, uint32_t cnt)
{
    const uint4 *qp = reinterpret_cast<const uint4 *>((uintptr_t)p & ~(uintptr_t)15);
    const uint32_t mis16 = (uint32_t)(uintptr_t)p & 15u, sh = (mis16 & 3u) * 8u;
    const uint32_t m1 = (mis16 & 4u) ? ~0u : 0u, m2 = (mis16 & 8u) ? ~0u : 0u;
    const uint32_t span = cnt ? mis16 + cnt : 0u;
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = make_uint4(0, 0, 0, 0);
    if (span > 0) q0 = qp[0];
    if (span > 16) q1 = qp[1];
    const uint32_t W[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
    uint32_t Aw[7], Bw[5];
#pragma unroll
    for (int j = 0; j < 7; ++j) Aw[j] = __builtin_amdgcn_bitop3_b32(W[j], W[j + 1], m1, 0xD8);      // m1 ? W[j + 1] : W[j]
#pragma unroll
    for (int j = 0; j < 5; ++j) Bw[j] = __builtin_amdgcn_bitop3_b32(Aw[j], Aw[j + 2], m2, 0xD8);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int32_t rem = (int32_t)cnt - 4 * j;
        const uint32_t keep = rem >= 4 ? ~0u : rem <= 0 ? 0u : (1u << (8 * rem)) - 1u;
        x[j] = __builtin_amdgcn_alignbit(Bw[j + 1], Bw[j], sh) & keep;
    }
}

// the first cnt <= 16 octets of y to q (any alignment): aligned dwords whose four octets are all the block's go out whole, the
// octets before the first and after the last such dword one by one; nothing is read-modify-written (bash_prg_ragged_kernel)
__device__ __forceinline__ void ae_store(uint8_t *q, const uint32_t (&y)[4], uint32_t cnt)
{
    const uint32_t md = (uint32_t)(uintptr_t)q & 3u, fsh = (32u - 8u * md) & 31u, m0 = md ? 0u : ~0u;
    uint8_t *qa = q - md;
    const uint32_t end = md + cnt, kt = end >> 2, tb = end & 3u;
    uint32_t z0 = 0, zt = 0;
#pragma unroll
    for (uint32_t k = 0; k < 5; ++k) {
        const uint32_t hi = k < 4 ? y[k] : 0u, lo = k ? y[k - 1] : 0u;
        const uint32_t z = __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_alignbit(hi, lo, fsh), hi, m0, 0xD8);    // md ? hi:lo >> .. : hi
        if (k == 0) z0 = z;
        else zt = k == kt ? z : zt;
        if (k < kt && (k || md == 0)) reinterpret_cast<uint32_t *>(qa)[k] = z;
    }
    if (md || kt == 0) {
#pragma unroll
        for (uint32_t b = 0; b < 4; ++b)
            if (b >= md && b < end) qa[b] = (uint8_t)(z0 >> (8 * b));
    }
    if (kt && tb) {
#pragma unroll
        for (uint32_t b = 0; b < 3; ++b)
            if (b < tb) qa[4 * kt + b] = (uint8_t)(zt >> (8 * b));
    }
}

// One lane per record.  A record is a fixed sequence of turns, each at most one E_K and then at most one product t <- (t ^ B) r:
//     iv -> s = E(iv)                       [dwp: r = E(s)]     r's table is built             (belt_dwp.c:44-62, belt_che.c:47-66)
//     header blocks B (the last zero-padded)               no E,  product                      (:103-145, :115-157)
//     text block j = 1, 2 ..: gamma = E(s + j) [che: E(S_j), S_j = S_{j-1} x ^ 1], out = in ^ gamma, B = the CIPHERTEXT block
//                             (the output of wrap, the input of unwrap; the last zero-padded)   (:64-101, :68-113, :159-211)
//     B = bits(header) || bits(text)                       no E,  product                      (:168-190, :218-239)
//     tag = E(t)[0..8)                                      E,    no product
// so E_K and the product are in the kernel once each, and a lane that has nothing to encrypt in a turn (a header block beside a
// neighbour's text block) waits for the others.  No branch and no global address depends on the key, s, r, t or the text:
// lengths, offsets, alignments and the verdict of unwrap are public; the tag comparison ORs all 8 differences.
// LDS: the multiplier's table index shows in no LDS cycle (GfLaneTab), the S-box index does -- BeltTabSmall is one shared 4 KiB
// table whose bank conflicts follow the bytes the 64 lanes look up together; it was chosen for occupancy.
__global__ __launch_bounds__(AE_WG, 2)
void belt_ae_ragged_kernel(const BeltAeArgs A, const uint8_t *ivs, const uint8_t *hdrs, const uint64_t *__restrict__ hoff,
                           const uint8_t *src, const uint64_t *__restrict__ off, const uint32_t *__restrict__ order, size_t n,
                           uint8_t *dst, uint8_t *tags, uint32_t *__restrict__ codes)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    AeTab::fill(smem, threadIdx.x, AE_WG);
    __syncthreads();
    const AeTab T(smem);
    const GfLaneTab M(smem + AeTab::kBytes);
    const size_t slot = (size_t)blockIdx.x * AE_WG + threadIdx.x;
    if (slot >= n) return;
    const size_t i = order ? order[slot] : slot;      // lane `slot` runs record order[slot]
    if (i >= n) return;
    uint32_t K[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) K[k] = A.key.k[k];
    const uint64_t h0 = hoff ? hoff[i] : 0, hlen = hoff ? hoff[i + 1] - h0 : 0;
    const uint64_t o0 = off[i], tlen = off[i + 1] - o0;
    enum : uint32_t { START = 0, START2 = 1, HEADER = 2, TEXT = 3, LENGTHS = 4, TAG = 5 };
    uint32_t ph = START;
    BeltCtr s = {{0, 0, 0, 0}};
    Gf128 S = {0, 0};                                 // che: the running S_j
    Gf128 t = gf_from(make_uint4(A.t0[0], A.t0[1], A.t0[2], A.t0[3]));
    const uint8_t *p = ivs + 16 * i;
    uint8_t *q = nullptr;
    uint64_t left = 16, j = 0;
    uint32_t x[4] = {0, 0, 0, 0};
    for (;;) {
        const uint32_t cnt = left < 16 ? (uint32_t)left : 16u;
        uint32_t blk[4] = {0, 0, 0, 0};
        if (ph == START || ph == HEADER || ph == TEXT) ae_load(blk, p, cnt);
        if (ph != HEADER && ph != LENGTHS) {
            if (ph == START) {
#pragma unroll
                for (int k = 0; k < 4; ++k) x[k] = blk[k];
            } else if (ph == START2) {
#pragma unroll
                for (int k = 0; k < 4; ++k) x[k] = s.c[k];
            } else if (ph == TEXT) {
                ++j;
                if (A.mode == 0) ctr_at(x, s, j);
                else {
                    S = gf_mul_xk(S, 1);
                    S.lo ^= 1;
                    x[0] = (uint32_t)S.lo; x[1] = (uint32_t)(S.lo >> 32); x[2] = (uint32_t)S.hi; x[3] = (uint32_t)(S.hi >> 32);
                }
            } else {
                x[0] = (uint32_t)t.lo; x[1] = (uint32_t)(t.lo >> 32); x[2] = (uint32_t)t.hi; x[3] = (uint32_t)(t.hi >> 32);
            }
            belt_encr(T, x, K);
        }
        if (ph == TAG) break;
        uint32_t go = 0;                                                         // 1: on to the header, 2: on to the text
        if (ph == START || ph == START2) {
            if (ph == START) {
#pragma unroll
                for (int k = 0; k < 4; ++k) s.c[k] = x[k];
                S = gf_from(make_uint4(x[0], x[1], x[2], x[3]));
            }
            if (ph == START && A.mode == 0) ph = START2;
            else {                                                               // r = x
                M.build(gf_from(make_uint4(x[0], x[1], x[2], x[3])));
                go = 1;
            }
        } else if (ph == LENGTHS) {
            t.lo ^= hlen * 8;
            t.hi ^= tlen * 8;
            t = M.mul(t);
            ph = TAG;
        } else {                                                                 // HEADER, TEXT
            if (ph == TEXT) {
                uint32_t y[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int32_t rem = (int32_t)cnt - 4 * k;
                    const uint32_t keep = rem >= 4 ? ~0u : rem <= 0 ? 0u : (1u << (8 * rem)) - 1u;
                    y[k] = blk[k] ^ (x[k] & keep);
                }
                ae_store(q, y, cnt);
                if (!A.unwrap) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) blk[k] = y[k];
                }
                q += 16;
            }
            t.lo ^= (uint64_t)blk[0] | (uint64_t)blk[1] << 32;
            t.hi ^= (uint64_t)blk[2] | (uint64_t)blk[3] << 32;
            t = M.mul(t);
            p += 16; left -= cnt;
            if (left == 0) go = ph == HEADER ? 2 : 3;
        }
        if (go == 1) {
            if (hlen) { ph = HEADER; p = hdrs + h0; left = hlen; }
            else go = 2;
        }
        if (go == 2) {
            if (tlen) { ph = TEXT; p = src + o0; q = dst + o0; left = tlen; }
            else go = 3;
        }
        if (go == 3) ph = LENGTHS;
    }
    uint8_t *tg = tags + 8 * i;
    if (!A.unwrap) {
#pragma unroll
        for (uint32_t b = 0; b < 8; ++b) tg[b] = (uint8_t)(x[b / 4] >> (8 * (b & 3)));
        return;
    }
    uint32_t diff = 0;
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b) diff |= (uint32_t)tg[b] ^ ((x[b / 4] >> (8 * (b & 3))) & 0xFFu);
    codes[i] = diff ? (uint32_t)ERR_BAD_MAC : (uint32_t)ERR_OK;
    if (diff) {                                       // a refused record keeps no plaintext: zeros over its own octets only
        uint8_t *z = dst + o0;
        size_t len = (size_t)tlen;
        for (; len && ((uintptr_t)z & 3u); ++z, --len) *z = 0;
        for (; len >= 4; z += 4, len -= 4) *reinterpret_cast<uint32_t *>(z) = 0;
        for (; len; ++z, --len) *z = 0;
    }
}

err_t launch_belt_ae_ragged(const BeltAeArgs &A, const void *d_ivs, const void *d_hdrs, const void *d_hoff, const void *d_src,
                            const void *d_off, const void *d_order, size_t n, void *d_dst, void *d_tags, void *d_codes, hipStream_t st)
{
    if (n == 0) return ERR_OK;
    if (n > 0xffffffffull) return ERR_BAD_INPUT;
    const uint32_t *ord = (const uint32_t *)d_order;
    if (!ord) {
        const err_t code = ragged_launch_order((const uint64_t *)d_off, n, st, &ord);
        if (code != ERR_OK) return code;
    }
    B2H_TRY(dyn_lds_once(reinterpret_cast<const void *>(belt_ae_ragged_kernel), AE_LDS));
    hipLaunchKernelGGL(belt_ae_ragged_kernel, dim3((unsigned)((n + AE_WG - 1) / AE_WG)), dim3(AE_WG), AE_LDS, st, A,
                       (const uint8_t *)d_ivs, (const uint8_t *)d_hdrs, (const uint64_t *)d_hoff, (const uint8_t *)d_src,
                       (const uint64_t *)d_off, ord, n, (uint8_t *)d_dst, (uint8_t *)d_tags, (uint32_t *)d_codes);
    B2H_TRY(hipGetLastError());
    return ERR_OK;
}

}  // namespace bee2hip
