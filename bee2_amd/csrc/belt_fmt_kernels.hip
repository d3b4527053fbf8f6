// belt_fmt_kernels.hip -- belt-fmt (STB 34.101.31, format-preserving encryption; src/crypto/belt/belt_fmt.c) over a batch of
// records that share (mod, count) and the key, one record per lane.  Device side of bee2hip_beltFMT_batch* (capi_fmt.hip).
// Part of bee2hip_tu_belt.hip, after belt_kernels.hip (BeltKey, dyn_lds_once).
#pragma once
#include "belt_dev.hpp"
#include "belt_fmt_common.hpp"
#include "common.hpp"

namespace bee2hip {

// what a launch is told by value (the key never sits in device memory the library does not own)
struct BeltFmtArgs {
    BeltKey key;
    uint32_t hw[6];         // beltH()[0..24) as six words: word 2 i + w serves step w of round i
    uint32_t hdr;           // u16le(mod & 0xffff) || u16le(count)
    FmtDiv div;             // mod and floor(2^32 / mod)
    uint32_t fl;            // floor(log2(mod))
    uint32_t decr;
    uint32_t count, n1, n2, b1, b2;
    uint32_t num_bytes;     // LDS of one wavefront's numbers: 256 (2 max(b1, b2) + 2)
    uint32_t wave_bytes;    // ... and of everything a wavefront owns: the numbers, then its 64 records
};

constexpr int FMT_WG_MAX = 256;                         // up to four wavefronts; the host picks 4, 2 or 1 so that the LDS fits
typedef BeltTabSmall FmtTab;                            // 4 KiB shared table, as the belt-AE record kernel

// Every record of a launch has the same (mod, count), so every loop bound below is the same in all 64 lanes and in every
// wavefront: no divergence, and no branch or address depends on the key, the iv, a symbol or a number.
//
// LDS of a wavefront:
//   the number   [limb][lane] dwords -- limb j of lane l is dword 64 j + l: the limb index is uniform, so lane l always sits
//                on bank l and no ds_read_b32 / ds_write_b32 has a bank conflict; up to 2 b + 2 = 152 limbs;
//   the records  [symbol][lane] u16 -- symbol s of lane l is halfword 64 s + l; two lanes share a dword, never two dwords a
//                bank.  The 64 records of a wavefront are 128 count contiguous octets of global memory: they come in and go
//                out as whole rows of 64 consecutive halfwords (coalesced; the pointers are only 2-aligned) and are
//                transposed on the way through this slab.  All six steps run on the slab.
// A step (belt_fmt.c:351-376) turns one half of the record into a number by Horner's rule, appends two words, encrypts the
// 8 b + 8 octets -- one E_K, belt-32block or belt-wbl -- and takes the other half's symbols out of the result by repeated
// division.  The cipher part is one loop with ONE E_K inside: b = 1 is one turn, belt-32block three (belt_fmt.c:157-175),
// belt-wbl 2 ceil(len / 16) (belt_wbl.c:50-82, the plain shifting form: sum and shift are one pass over the limbs, and the
// length may be 8 mod 16).
__global__ __launch_bounds__(FMT_WG_MAX)
void belt_fmt_batch_kernel(const BeltFmtArgs A, const uint8_t *__restrict__ ivs, const uint16_t *src, size_t n, uint16_t *dst)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    FmtTab::fill(smem, threadIdx.x, blockDim.x);
    __syncthreads();
    const FmtTab T(smem);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const size_t g0 = ((size_t)blockIdx.x * waves + wave) * 64;          // the wavefront's first record
    if (g0 >= n) return;                                                 // (whole wavefronts only; no barrier follows)
    uint8_t *mine = smem + FmtTab::kBytes + wave * A.wave_bytes;
    uint32_t *const num = reinterpret_cast<uint32_t *>(mine) + lane;
    uint16_t *const slab = reinterpret_cast<uint16_t *>(mine + A.num_bytes);
    uint16_t *const sym = slab + lane;
    const uint32_t count = A.count;
    const uint32_t nrec = n - g0 < 64 ? (uint32_t)(n - g0) : 64u;
    const uint32_t elems = nrec * count;

    // records in: halfword e of the wavefront's range is symbol e mod count of record e / count
    {
        const uint16_t *p = src + g0 * count;
        const uint32_t dq = 64u / count, dr = 64u % count;
        uint32_t r = lane / count, s = lane % count;
        for (uint32_t e = lane; e < elems; e += 64) {
            slab[64 * s + r] = p[e];
            r += dq; s += dr;
            if (s >= count) { s -= count; ++r; }
        }
    }
    uint32_t iv0 = 0, iv1 = 0, iv2 = 0, iv3 = 0;
    if (ivs && lane < nrec) {                                            // any alignment: octet by octet
        const uint8_t *q = ivs + 16 * (g0 + lane);
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            w[k] = (uint32_t)q[4 * k] | (uint32_t)q[4 * k + 1] << 8 | (uint32_t)q[4 * k + 2] << 16 | (uint32_t)q[4 * k + 3] << 24;
        iv0 = w[0]; iv1 = w[1]; iv2 = w[2]; iv3 = w[3];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();

    uint32_t K[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) K[k] = A.key.k[k];
    const FmtDiv D = A.div;
    const bool pow16 = D.mod == 65536u;

    for (uint32_t t = 0; t < 6; ++t) {
        const uint32_t step = A.decr ? 5u - t : t;                       // 2 i + w of belt_fmt.c:351 (encryption order)
        const bool second = (step & 1u) != 0;
        // first step of a round: the number of the right half goes into the left one; second: the other way round
        const uint32_t in_off = second ? 0u : A.n1, in_cnt = second ? A.n1 : A.n2, b = second ? A.b1 : A.b2;
        const uint32_t out_off = second ? A.n1 : 0u, out_cnt = second ? A.n2 : A.n1;
        const uint32_t nl = 2u * b, L = nl + 2u;
        const uint16_t *in = sym + 64u * in_off;
        uint16_t *out = sym + 64u * out_off;

        // ---- the number: sum in[j] mod^j modulo 2^(64 b).  After k symbols it is below 2^(16 k): ceil(k / 2) limbs are live
        if (pow16) {
            const uint32_t full = in_cnt >> 1;
            for (uint32_t j = 0; j < full; ++j) num[64 * j] = (uint32_t)in[64 * (2 * j)] | (uint32_t)in[64 * (2 * j + 1)] << 16;
            uint32_t used = full;
            if (in_cnt & 1u) { num[64 * full] = in[64 * (in_cnt - 1)]; used = full + 1; }
            for (uint32_t j = used; j < nl; ++j) num[64 * j] = 0;
        } else {
            num[0] = in[64 * (in_cnt - 1)];
            uint32_t used = 1;
            for (uint32_t k = 2; k <= in_cnt; ++k) {
                uint32_t carry = in[64 * (in_cnt - k)];
                for (uint32_t j = 0; j < used; ++j) {
                    const uint64_t p = (uint64_t)num[64 * j] * D.mod + carry;
                    num[64 * j] = (uint32_t)p;
                    carry = (uint32_t)(p >> 32);
                }
                const uint32_t want = (k + 1) >> 1 < nl ? (k + 1) >> 1 : nl;
                if (want > used) { num[64 * used] = carry; used = want; }
            }
            for (uint32_t j = used; j < nl; ++j) num[64 * j] = 0;
        }
        {
            uint32_t ivw = A.hdr;                                        // iv' = hdr || iv || hdr, word `step`
            ivw = step == 1 ? iv0 : ivw;
            ivw = step == 2 ? iv1 : ivw;
            ivw = step == 3 ? iv2 : ivw;
            ivw = step == 4 ? iv3 : ivw;
            uint32_t hw = A.hw[0];                                       // (selects: a run-time index would put the array in scratch)
#pragma unroll
            for (uint32_t k = 1; k < 6; ++k) hw = step == k ? A.hw[k] : hw;
            num[64 * nl] = hw;
            num[64 * (nl + 1)] = ivw;
        }

        // ---- the cipher on L = 2 b + 2 limbs
        const uint32_t turns = b == 1 ? 1u : b == 2 ? 3u : 2u * ((L + 3u) >> 2);
        for (uint32_t r = 1; r <= turns; ++r) {
            uint32_t x[4];
            uint32_t base = 0;
            if (b == 1) {
#pragma unroll
                for (int k = 0; k < 4; ++k) x[k] = num[64 * k];
            } else if (b == 2) {
                base = r == 1 ? 2u : r == 2 ? 4u : 0u;
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    const uint32_t i = base + k;
                    x[k] = num[64 * (i >= 6 ? i - 6 : i)];
                }
            } else {
                // s = the sum of the whole blocks at limbs 0, 4 .. while that block's end is before L; the buffer moves down
                // by four limbs; s becomes the last block
#pragma unroll
                for (int k = 0; k < 4; ++k) x[k] = num[64 * k];
                uint32_t blk = 4;
                for (; blk + 4 <= L; blk += 4) {
                    uint32_t v[4];
#pragma unroll
                    for (uint32_t k = 0; k < 4; ++k) v[k] = num[64 * (blk + k)];
                    if (blk + 4 < L) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) x[k] ^= v[k];
                    }
#pragma unroll
                    for (uint32_t k = 0; k < 4; ++k) num[64 * (blk - 4 + k)] = v[k];
                }
                if (blk < L) {                                           // two limbs left: the length is 8 mod 16
                    const uint32_t v0 = num[64 * blk], v1 = num[64 * (blk + 1)];
                    num[64 * (blk - 4)] = v0;
                    num[64 * (blk - 3)] = v1;
                }
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) num[64 * (L - 4 + k)] = x[k];
            }
            belt_encr(T, x, K);
            if (b == 1) {
#pragma unroll
                for (int k = 0; k < 4; ++k) num[64 * k] = x[k];
            } else if (b == 2) {
                x[0] ^= r;
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    const uint32_t i = base + k;
                    num[64 * (i >= 6 ? i - 6 : i)] = x[k];
                }
                const uint32_t i0 = base >= 2 ? base - 2 : base + 4;     // the two words before the block, cyclically
                num[64 * i0] ^= x[0];
                num[64 * (i0 + 1)] ^= x[1];
            } else {
                x[0] ^= r;
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) num[64 * (L - 8 + k)] ^= x[k];
            }
        }

        // ---- the symbols of the other half: s <- (s +- a mod mod) mod mod, a <- a div mod
        if (pow16) {
            for (uint32_t k = 0; k < out_cnt; ++k) {
                const uint32_t piece = (num[64 * (k >> 1)] >> (16u * (k & 1u))) & 0xFFFFu;
                const uint32_t s = out[64 * k];
                out[64 * k] = (uint16_t)(A.decr ? s - piece : s + piece);
            }
        } else {
            for (uint32_t k = 0; k < out_cnt; ++k) {
                // a < 2^(32 L - k floor(log2 mod)) by now: the limbs above that are zero
                const uint32_t gone = k * A.fl, bits = 32u * L > gone ? 32u * L - gone : 1u;
                const uint32_t live = (bits + 31u) >> 5;
                uint32_t rem = 0;
                for (uint32_t j = live; j-- > 0;) {
                    const uint32_t v = num[64 * j];
                    uint32_t qh, ql;
                    rem = fmt_divstep(rem, v >> 16, D, &qh);
                    rem = fmt_divstep(rem, v & 0xFFFFu, D, &ql);
                    num[64 * j] = qh << 16 | ql;
                }
                const uint32_t s = out[64 * k];
                uint32_t q;
                out[64 * k] = (uint16_t)fmt_divmod(s + (A.decr ? D.mod - rem : rem), D, &q);
            }
        }
    }

    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // records out: the same rows; only the records' own octets are written
    {
        uint16_t *p = dst + g0 * count;
        const uint32_t dq = 64u / count, dr = 64u % count;
        uint32_t r = lane / count, s = lane % count;
        for (uint32_t e = lane; e < elems; e += 64) {
            p[e] = slab[64 * s + r];
            r += dq; s += dr;
            if (s >= count) { s -= count; ++r; }
        }
    }
}

static_assert(FmtTab::kBytes == FMT_TAB_BYTES, "fmt_plan() counts the table the kernel fills");

// key: expanded; H: the S-box octets (host); d_ivs may be null (all zero)
err_t launch_belt_fmt_batch(int decr, uint32_t mod, size_t count, const uint32_t key[8], const uint8_t *H, const void *d_ivs,
                            const void *d_src, size_t n, void *d_dst, hipStream_t st)
{
    if (n == 0) return ERR_OK;
    if (n > 0xffffffffull || mod < 2 || mod > FMT_MOD_MAX || count < 2 || count > FMT_COUNT_MAX) return ERR_BAD_INPUT;
    BeltFmtArgs A;
    memset(&A, 0, sizeof A);
    for (int k = 0; k < 8; ++k) A.key.k[k] = key[k];
    for (int k = 0; k < 6; ++k)
        A.hw[k] = (uint32_t)H[4 * k] | (uint32_t)H[4 * k + 1] << 8 | (uint32_t)H[4 * k + 2] << 16 | (uint32_t)H[4 * k + 3] << 24;
    A.hdr = (mod & 0xFFFFu) | (uint32_t)count << 16;
    A.div = fmt_div_make(mod);
    A.fl = fmt_floor_log2(mod);
    A.decr = decr ? 1u : 0u;
    A.count = (uint32_t)count;
    A.n1 = (uint32_t)((count + 1) / 2);
    A.n2 = (uint32_t)(count / 2);
    const FmtPlan P = fmt_plan(mod, count);                              // (belt_fmt_common.hpp: 4, 2 or 1 wavefronts)
    A.b1 = P.b1;
    A.b2 = P.b2;
    A.num_bytes = P.num_bytes;
    A.wave_bytes = P.wave_bytes;
    B2H_TRY(dyn_lds_once(reinterpret_cast<const void *>(belt_fmt_batch_kernel), P.lds));
    const size_t per_wg = 64 * (size_t)P.waves;
    hipLaunchKernelGGL(belt_fmt_batch_kernel, dim3((unsigned)((n + per_wg - 1) / per_wg)), dim3(64 * P.waves), P.lds, st, A,
                       (const uint8_t *)d_ivs, (const uint16_t *)d_src, n, (uint16_t *)d_dst);
    B2H_TRY(hipGetLastError());
    return ERR_OK;
}

}  // namespace bee2hip
