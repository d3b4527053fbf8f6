// belt_hmac_kernels.hip -- belt-hmac and belt-pbkdf2 (STB 34.101.31; src/crypto/belt/belt_hmac.c, belt_pbkdf.c) over a batch of
// records, one record per lane.  Device side of bee2hip_beltHMAC_*ragged* and bee2hip_beltPBKDF2_batch* (capi_hmac.hip).  Part of
// bee2hip_tu_belt.hip, after belt_kernels.hip.  ONE lane per record whatever its length: long messages in several lanes
// (belt_hash_long_kernel's forms) are not served here.
#pragma once
#include "belt_dev.hpp"
#include "belt_hmac_common.hpp"
#include "common.hpp"

namespace bee2hip {

// what is the same for every record of a launch
struct HmacArgs {
    HmacKeyState ks;                // shared != 0: the state of the batch's one key, computed on the host
    uint32_t shared, suffix, iter, mac_len, verify;
    uint64_t msg_len, msg_stride;   // off == NULL: message i = data + i * msg_stride, msg_len octets
};

// One source of octets at any alignment, read as belt_hash_ragged_kernel reads its messages: the aligned 16-octet quads that
// hold a block's octets, brought into place by a dword shift (mask selects) and v_alignbit.
struct HmacSrc {
    const uint4 *qp;
    uint32_t mis16;
    __device__ __forceinline__ explicit HmacSrc(const uint8_t *p)
        : qp(reinterpret_cast<const uint4 *>((uintptr_t)p & ~(uintptr_t)15)), mis16((uint32_t)(uintptr_t)p & 15u) {}
};
struct HmacReader {
    HmacSrc key, msg;
    __device__ __forceinline__ void block(uint32_t (&X)[8], uint32_t is_key, uint64_t blk, uint32_t cnt) const
    {
        const uint4 *qp = (is_key ? key.qp : msg.qp) + 2 * blk;
        const uint32_t mis16 = is_key ? key.mis16 : msg.mis16, sh = (mis16 & 3u) * 8u;
        const uint32_t m1 = (mis16 & 4u) ? ~0u : 0u, m2 = (mis16 & 8u) ? ~0u : 0u;
        // aligned quad j holds octets of the block iff the block has any and 16 j < span: a quad without an octet of the
        // record is never loaded (a record may end where its allocation ends)
        const uint32_t span = cnt ? mis16 + cnt : 0u;
        uint32_t W[16];
#pragma unroll
        for (uint32_t j = 0; j < 3; ++j) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (16u * j < span) v = qp[j];
            W[4 * j] = v.x; W[4 * j + 1] = v.y; W[4 * j + 2] = v.z; W[4 * j + 3] = v.w;
        }
        W[12] = W[13] = W[14] = W[15] = 0;
        uint32_t A[11], B[9];
#pragma unroll
        for (uint32_t j = 0; j < 11; ++j) A[j] = __builtin_amdgcn_bitop3_b32(W[j], W[j + 1], m1, 0xD8);     // m1 ? W[j + 1] : W[j]
#pragma unroll
        for (uint32_t j = 0; j < 9; ++j) B[j] = __builtin_amdgcn_bitop3_b32(A[j], A[j + 2], m2, 0xD8);
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) X[j] = __builtin_amdgcn_alignbit(B[j + 1], B[j], sh);
    }
};
struct HmacCompress {
    const BeltTabSmall &T;
    __device__ __forceinline__ void operator()(uint32_t (&s1)[4], uint32_t (&h)[8], const uint32_t (&X)[8]) const
    {
        belt_compress(T, s1, h, X);
    }
};

// Lane k of the launch serves record order[k] (or k).  Keys: A.shared, or key i = keys[key_off[i] .. key_off[i + 1]).
// Messages: data[off[i] .. off[i + 1]), or with off == NULL data + i * A.msg_stride, A.msg_len octets.  macs: A.mac_len octets a
// record at any alignment, written (verify = 0) or compared into codes (verify = 1).  The table sits in static shared memory
// (look-up addresses with immediate offsets, as belt_hash_ragged_kernel).
__global__ __launch_bounds__(64)
void belt_hmac_batch_kernel(const HmacArgs A, const uint8_t *__restrict__ keys, const uint64_t *__restrict__ key_off,
                            const uint8_t *__restrict__ data, const uint64_t *__restrict__ off,
                            const uint32_t *__restrict__ order, const size_t n, uint8_t *macs, uint32_t *__restrict__ codes)
{
    __shared__ __attribute__((aligned(16))) uint8_t smem[BeltTabSmall::kBytes];
    BeltTabSmall::fill(smem, threadIdx.x, 64);
    __syncthreads();
    const BeltTabSmall Tab(smem);
    const size_t slot = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (slot >= n) return;
    const size_t i = order ? order[slot] : slot;
    uint32_t H0[8];
#pragma unroll
    for (int k = 0; k < 8; ++k)
        H0[k] = (uint32_t)c_beltH[4 * k] | (uint32_t)c_beltH[4 * k + 1] << 8 | (uint32_t)c_beltH[4 * k + 2] << 16 |
                (uint32_t)c_beltH[4 * k + 3] << 24;
    const uint8_t *kp = nullptr, *mp;
    uint64_t key_len = 0, msg_len;
    if (!A.shared) { kp = keys + key_off[i]; key_len = key_off[i + 1] - key_off[i]; }
    if (off) { mp = data + off[i]; msg_len = off[i + 1] - off[i]; }
    else { mp = data + i * A.msg_stride; msg_len = A.msg_len; }
    HmacKeyState ks = A.ks;
    const HmacReader rd{HmacSrc(kp), HmacSrc(mp)};
    const HmacCompress cf{Tab};
    uint32_t acc[8];
    hmac_lane(cf, rd, H0, ks, A.shared, key_len, msg_len, A.suffix, A.iter, acc);

    uint8_t *m = macs + i * A.mac_len;
    if (A.verify) {
        uint32_t M[8];
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            uint32_t v = 0;
#pragma unroll
            for (uint32_t b = 0; b < 4; ++b)
                if (4 * j + b < A.mac_len) v |= (uint32_t)m[4 * j + b] << (8 * b);
            M[j] = v;
        }
        codes[i] = hmac_differs(acc, M, A.mac_len) * HMAC_ERR_BAD_MAC;
        return;
    }
    if ((A.mac_len & 3u) == 0 && ((uintptr_t)macs & 3u) == 0) {          // whole dwords (the same way in every lane)
        uint32_t *m4 = reinterpret_cast<uint32_t *>(m);
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j)
            if (4 * j < A.mac_len) m4[j] = acc[j];
        return;
    }
#pragma unroll
    for (uint32_t b = 0; b < 32; ++b)
        if (b < A.mac_len) m[b] = (uint8_t)(acc[b >> 2] >> (8 * (b & 3)));
}

// d_order NULL and n >= 128: longest first by the lengths that make lanes differ -- the messages' when they are ragged, the
// keys' (the passwords of PBKDF2) when the messages have one length
err_t launch_belt_hmac_batch(const HmacArgs &A, const void *d_keys, const void *d_key_off, const void *d_data, const void *d_off,
                             const void *d_order, size_t n, void *d_macs, void *d_codes, hipStream_t st)
{
    if (n == 0) return ERR_OK;
    if (n > 0xffffffffull || A.iter == 0 || A.iter > HMAC_ITER_MAX || A.mac_len == 0 || A.mac_len > 32) return ERR_BAD_INPUT;
    const uint32_t *ord = (const uint32_t *)d_order;
    if (!ord) {
        const uint64_t *by = (const uint64_t *)(d_off ? d_off : d_key_off);
        if (by) {
            const err_t code = ragged_launch_order(by, n, st, &ord);
            if (code != ERR_OK) return code;
        }
    }
    hipLaunchKernelGGL(belt_hmac_batch_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, A, (const uint8_t *)d_keys,
                       (const uint64_t *)d_key_off, (const uint8_t *)d_data, (const uint64_t *)d_off, ord, n, (uint8_t *)d_macs,
                       (uint32_t *)d_codes);
    B2H_TRY(hipGetLastError());
    return ERR_OK;
}

}  // namespace bee2hip
