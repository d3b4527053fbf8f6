// belt_kwp_kernels.hip -- belt-kwp (STB 34.101.31, key wrap; src/crypto/belt/belt_kwp.c = belt-wbl over key || header) over a
// batch of records that share the length, one record per lane, under one key for the batch or one key per record.  Device
// side of bee2hip_beltKWP_*batch* (capi_kwp.hip) and of the bpki containers (capi_bpki.hip).  Part of bee2hip_tu_belt.hip, after
// belt_kernels.hip (BeltKey, dyn_lds_once).
#pragma once
#include "belt_dev.hpp"
#include "belt_kwp_common.hpp"
#include "common.hpp"

namespace bee2hip {

constexpr int KWP_WG_MAX = 256;                         // up to four wavefronts; the host picks 4, 2 or 1 so that the LDS fits
typedef BeltTabSmall KwpTab;                            // 4 KiB shared table, as the other record kernels
static_assert(KwpTab::kBytes == KWP_TAB_BYTES, "kwp_plan() counts the table");

struct KwpColumn {                                      // a lane's column of the [dword][lane] slab: dword j of lane l is dword 64 j + l
    uint32_t *p;
    __device__ __forceinline__ uint32_t ld(uint32_t j) const { return p[64u * j]; }
    __device__ __forceinline__ void st(uint32_t j, uint32_t v) { p[64u * j] = v; }
};
struct KwpEK {
    const KwpTab &T;
    const uint32_t (&K)[8];
    __device__ __forceinline__ void operator()(uint32_t (&x)[4]) const { belt_encr(T, x, K); }
};

// Every record of a launch has the same token size T, so every trip count and every LDS index below is the same in all 64
// lanes and in every wavefront: no divergence, and no branch or address depends on the key, a header or a record.
//
// LDS of a wavefront: the tokens as [dword][lane] -- dword j of lane l is dword 64 j + l, the dword index is uniform, so lane
// l always sits on bank l and no ds_read_b32 / ds_write_b32 of the rounds has a bank conflict; ceil(T / 4) dwords a lane,
// 64 KiB at T = 1024.  A token sits END-aligned in its column (belt_kwp_common.hpp says why and what that does to the rounds,
// which are kwp_lane() there, shared with the tests' CPU build).
// The 64 records of a wavefront are 64 in_len contiguous octets of global memory: they come in as whole rows of consecutive
// octets -- dwords when the base is 4-aligned and the length a multiple of 4 -- and are transposed on the way into the slab;
// results go out the same way, only the records' own octets, so that a partial last wavefront touches nothing behind them.
//
// Two instantiations.  KEYED = false is the batch under one key, whose expanded words travel in `key` and stay in scalar
// registers: its text is what it was before the keyed form came (the two arguments behind `codes` are not looked at).  KEYED =
// true takes one key per record from `keys` (DESIGN.md 4.17 says why it is not one kernel with a null test).
template <bool KEYED>
__global__ __launch_bounds__(KWP_WG_MAX)
void belt_kwp_batch_kernel(const BeltKey key, const uint32_t T, const uint32_t unwrap, const uint32_t wave_bytes,
                           const uint8_t *__restrict__ hdrs, const uint8_t *__restrict__ src, const size_t n,
                           uint8_t *__restrict__ dst, uint32_t *__restrict__ codes, const uint8_t *__restrict__ keys,
                           const uint32_t key_len)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    KwpTab::fill(smem, threadIdx.x, blockDim.x);
    __syncthreads();
    const KwpTab Tab(smem);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const size_t g0 = ((size_t)blockIdx.x * waves + wave) * 64;          // the wavefront's first record
    if (g0 >= n) return;                                                 // (whole wavefronts only; no barrier follows)
    uint8_t *const slab8 = smem + KwpTab::kBytes + wave * wave_bytes;
    uint32_t *const slab = reinterpret_cast<uint32_t *>(slab8);
    const uint32_t nrec = n - g0 < 64 ? (uint32_t)(n - g0) : 64u;
    const uint32_t in_len = unwrap ? T : T - 16u, out_len = unwrap ? T - 16u : T;
    const uint32_t pad = kwp_pad(T);

    // records in: octet e of the wavefront's range is octet e mod in_len of record e / in_len
    {
        const uint8_t *p = src + g0 * in_len;
        if (pad == 0 && ((uintptr_t)p & 3u) == 0) {
            const uint32_t *p4 = reinterpret_cast<const uint32_t *>(p);
            const uint32_t len4 = in_len >> 2, elems = nrec * len4;
            const uint32_t dq = 64u / len4, dr = 64u % len4;
            uint32_t r = lane / len4, j = lane % len4;
B2H_ROLLED
            for (uint32_t e = lane; e < elems; e += 64) {
                slab[64u * j + r] = p4[e];
                r += dq; j += dr;
                if (j >= len4) { j -= len4; ++r; }
            }
        } else {
            const uint32_t elems = nrec * in_len;
            const uint32_t dq = 64u / in_len, dr = 64u % in_len;
            uint32_t r = lane / in_len, b = lane % in_len;
B2H_ROLLED
            for (uint32_t e = lane; e < elems; e += 64) {
                slab8[kwp_slab_octet(T, r, b)] = p[e];
                r += dq; b += dr;
                if (b >= in_len) { b -= in_len; ++r; }
            }
        }
    }
    uint32_t hdr[4] = {0, 0, 0, 0};
    if (hdrs && lane < nrec) {                                           // any alignment: octet by octet
        const uint8_t *q = hdrs + 16 * (g0 + lane);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            hdr[k] = (uint32_t)q[4 * k] | (uint32_t)q[4 * k + 1] << 8 | (uint32_t)q[4 * k + 2] << 16 | (uint32_t)q[4 * k + 3] << 24;
    }
    // KEYED: the key_len octets of record g0 + lane, read as the header is and expanded by kwp_key_words() (belt_kwp_common.hpp:
    // the tests run it on the CPU).  Lanes past nrec take the zero key
    uint32_t K[8];
    if (KEYED) {
#pragma unroll
        for (int k = 0; k < 8; ++k) K[k] = 0u;
        if (lane < nrec) kwp_key_words(K, keys + (size_t)key_len * (g0 + lane), key_len);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();

    if (!KEYED) {
#pragma unroll
        for (int k = 0; k < 8; ++k) K[k] = key.k[k];
    }
    KwpColumn col{slab + lane};
    KwpEK ek{Tab, K};
    const uint32_t code = kwp_lane(col, ek, T, unwrap, hdr);             // (lanes past nrec work on what the slab held: LDS only)
    if (unwrap && lane < nrec) codes[g0 + lane] = code;

    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // records out: the same rows; only the records' own octets are written
    {
        uint8_t *p = dst + g0 * out_len;
        if (pad == 0 && ((uintptr_t)p & 3u) == 0) {
            uint32_t *p4 = reinterpret_cast<uint32_t *>(p);
            const uint32_t len4 = out_len >> 2, elems = nrec * len4;
            const uint32_t dq = 64u / len4, dr = 64u % len4;
            uint32_t r = lane / len4, j = lane % len4;
B2H_ROLLED
            for (uint32_t e = lane; e < elems; e += 64) {
                p4[e] = slab[64u * j + r];
                r += dq; j += dr;
                if (j >= len4) { j -= len4; ++r; }
            }
        } else {
            const uint32_t elems = nrec * out_len;
            const uint32_t dq = 64u / out_len, dr = 64u % out_len;
            uint32_t r = lane / out_len, b = lane % out_len;
B2H_ROLLED
            for (uint32_t e = lane; e < elems; e += 64) {
                p[e] = slab8[kwp_slab_octet(T, r, b)];
                r += dq; b += dr;
                if (b >= out_len) { b -= out_len; ++r; }
            }
        }
    }
}

// key: expanded, for the whole batch, or null with d_keys: n keys of key_len = 16, 24 or 32 octets, any alignment; count: the
// octets of a record of src (the key to wrap, or the token); d_hdrs may be null (all zero); d_codes: unwrap only
err_t launch_belt_kwp_batch(int unwrap, size_t count, const uint32_t key[8], const void *d_keys, size_t key_len, const void *d_hdrs,
                            const void *d_src, size_t n, void *d_dst, void *d_codes, hipStream_t st)
{
    if (n == 0) return ERR_OK;
    const size_t T = unwrap ? count : count + 16;
    if (n > 0xffffffffull || T < KWP_TOKEN_MIN || T > KWP_TOKEN_MAX || (unwrap && !d_codes)) return ERR_BAD_INPUT;
    if (!key == !d_keys || (d_keys && key_len != 16 && key_len != 24 && key_len != 32)) return ERR_BAD_INPUT;
    BeltKey k;
    for (int i = 0; i < 8; ++i) k.k[i] = key ? key[i] : 0u;
    const KwpPlan plan = kwp_plan((uint32_t)T);
    const auto kern = d_keys ? belt_kwp_batch_kernel<true> : belt_kwp_batch_kernel<false>;
    B2H_TRY(dyn_lds_once(reinterpret_cast<const void *>(kern), plan.lds));
    const size_t per_wg = 64 * (size_t)plan.waves;
    hipLaunchKernelGGL(kern, dim3((unsigned)((n + per_wg - 1) / per_wg)), dim3(64 * plan.waves), plan.lds, st, k, (uint32_t)T,
                       unwrap ? 1u : 0u, plan.wave_bytes, (const uint8_t *)d_hdrs, (const uint8_t *)d_src, n, (uint8_t *)d_dst,
                       (uint32_t *)d_codes, (const uint8_t *)d_keys, (uint32_t)key_len);
    B2H_TRY(hipGetLastError());
    return ERR_OK;
}

}  // namespace bee2hip
