// bash_prg_kernels.hip -- the programmable sponge algorithms of STB 34.101.77 (bash-prg: prg-hash, annex A.5, and prg-ae,
// annex A.6; src/crypto/bash/bash_prg.c) over a ragged batch of records, one automaton per record.  Device side of
// bee2hip_bashPrgHash_ragged* and bee2hip_bashPrgAE_*_ragged* (capi_prg.hip).  Part of bee2hip_tu_belt.hip, after
// mixed_kernels.hip (bash_f, the ragged launch order).
#pragma once
#include "bash_dev.hpp"
#include "common.hpp"
#include <type_traits>

namespace bee2hip {

// what a launch is told by value (the key never sits in device memory the library does not own)
struct BashPrgArgs {
    uint32_t fixed[15];     // AE: the key; prg-hash: the batch's announcement -- little-endian words, zeros behind
    uint32_t n_fixed;       // words of it
    uint32_t n_ann;         // words of a record's OWN announcement, read from anns + 4 n_ann i (prg-hash: 0)
    uint32_t head;          // octet 0 of the start state: ann_len * 4 + key_len / 4 (bash_prg.c:125)
    uint32_t cap;           // octet 184: l / 4 + d (bash_prg.c:131)
    uint32_t rate;          // buf_len (bash_prg.c:133), a multiple of 4 in 64 .. 168
    uint32_t mode;          // BASH_PRG_HASH / WRAP / UNWRAP
    uint32_t out_len;       // octets squeezed: the digest or the tag, 1 .. 64
};
enum : uint32_t { BASH_PRG_HASH = 0, BASH_PRG_WRAP = 1, BASH_PRG_UNWRAP = 2 };
constexpr uint32_t BASH_PRG_MAX_RATE = 168;        // (l, d) = (128, 1), keyed

// One lane per record, the automaton's 192 octets in registers.  A record is a fixed sequence of commands
// (bash_prg.c:89-102 commit, :182-209 absorb, :275-308 encr, :328-361 decr, :228-255 squeeze):
//     start; commit(DATA) absorb(header); [ commit(TEXT) encr / decr (text); ] commit(OUT) squeeze
// Every command begins at pos = 0 after its commit, so its data is whole rate blocks and a tail of 0 .. r - 1 octets, as in
// bash_ragged_kernel, and the commit that ends it xors the next command's code at octet `tail` and 0x80 at octet r before the
// permutation.  The loop below does ONE block per turn -- of the start state (nothing to load; its "tail" is 1 + |ann| + |key|),
// then of the header, then of the text -- so bash-f is in the kernel once; a lane leaves after the commit(OUT) permutation.
//   * a block is read as the aligned 16-octet quads that hold it and shifted into place by p mod 16 (bash_ragged_kernel); the
//     quad count is that of the largest rate, predicated by `span`; octets past the block are masked off, so a quad shared with
//     the neighbouring record -- even one the neighbour's lane has overwritten in place -- contributes only the record's own octets
//   * absorb XORS into the state (bash-hash overwrites); encr emits state ^ text and keeps it; decr emits state ^ text and keeps
//     the text in the first `cnt` octets: new = y ^ (old & keep & dec), y = old ^ x, for all three
//   * the rate is a launch argument and 156 is no multiple of 8: everything is done on 32-bit words S(j) = a[j / 2].lo / .hi
//   * stores: records are packed back to back, so only aligned dwords whose four octets are all the record's own are written
//     whole; the octets before the first and after the last such dword go out one by one.  Nothing is read-modify-written.
//   * no branch and no address depends on key, state or text: lengths, offsets, alignments and the verdict of unwrap are public.
//     The tag comparison ORs all out_len differences.
// hipcc -Rpass-analysis=kernel-resource-usage (gfx950): 113 VGPRs, 0 AGPRs, 106 SGPRs (38 of them parked in lanes of a VGPR),
// ScratchSize 0, no VGPR spill, 4 wavefronts per SIMD -- bash_ragged_kernel<16>: 108 VGPRs, 62 SGPRs, 4 wavefronts.  DESIGN.md 4.12.
__global__ __launch_bounds__(64, BASH_RAGGED_WAVES)
void bash_prg_ragged_kernel(const BashPrgArgs A, const uint8_t *__restrict__ anns,
                            const uint8_t *hdrs, const uint64_t *__restrict__ hoff,
                            const uint8_t *src, const uint64_t *__restrict__ off,
                            const uint32_t *__restrict__ order, size_t n,
                            uint8_t *dst, uint8_t *tags, uint32_t *__restrict__ codes)
{
    const size_t slot = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (slot >= n) return;
    const size_t i = order ? order[slot] : slot;      // lane `slot` runs record order[slot]
    if (i >= n) return;
    constexpr uint32_t NW = BASH_PRG_MAX_RATE / 4;    // 42 words: the largest rate
    constexpr uint32_t NQ = (15 + BASH_PRG_MAX_RATE + 15) / 16;      // 12 quads can hold octets of one block
    const uint32_t r = A.rate;
    u64x2 a[24];
#define S(j) (((j) & 1) ? a[(j) / 2].hi : a[(j) / 2].lo)
    // start state (bash_prg.c:122-131): head || ann || key || 0.., ann || key word-aligned in u[], one octet further in s
    {
        const uint32_t *my = reinterpret_cast<const uint32_t *>(anns) + (size_t)A.n_ann * i;
        uint32_t prev = A.head;
#pragma unroll
        for (uint32_t k = 0; k < 31; ++k) {
            uint32_t u = 0;
            if (k < A.n_ann) u = my[k];
            else if (k - A.n_ann < A.n_fixed) u = A.fixed[k - A.n_ann];
            S(k) = (u << 8) | prev;
            prev = u >> 24;
        }
#pragma unroll
        for (uint32_t k = 31; k < 48; ++k) S(k) = 0;
        a[23].lo = A.cap;
    }
    uint32_t ph = 0;                                  // 0 start, 1 header (prg-hash: the message), 2 text
    const uint8_t *p = nullptr;
    uint8_t *q = nullptr;
    size_t left = 0;
    for (;;) {
        const uint32_t cnt = left < r ? (uint32_t)left : r;             // octets of this block
        const bool last = cnt < r;                                      // the command ends here: commit
        const uint4 *qp = reinterpret_cast<const uint4 *>((uintptr_t)p & ~(uintptr_t)15);
        const uint32_t mis16 = (uint32_t)(uintptr_t)p & 15u, sh = (mis16 & 3u) * 8u;
        const uint32_t m1 = (mis16 & 4u) ? ~0u : 0u, m2 = (mis16 & 8u) ? ~0u : 0u;
        const uint32_t span = cnt ? mis16 + cnt : 0u;                   // aligned quad j holds octets of the block iff 16 j < span
        // The block goes through in six chunks of 8 words (the last: 2): the three quads a chunk draws on are shifted, masked,
        // folded into the state and -- for the text -- stored before the next chunk is touched, and the two new quads of chunk
        // c + 1 are requested before chunk c is worked.  All 12 quads at once, beside the 48 state words, do not fit 128 registers.
        uint4 Q[NQ];
        const auto ldq = [&](uint32_t j) {
            Q[j] = make_uint4(0, 0, 0, 0);
            if (16u * j < span) Q[j] = qp[j];
        };
        const auto Wq = [&](uint32_t j) -> uint32_t {
            return j >= 4 * NQ ? 0u : (j & 3) == 0 ? Q[j / 4].x : (j & 3) == 1 ? Q[j / 4].y : (j & 3) == 2 ? Q[j / 4].z : Q[j / 4].w;
        };
        const uint32_t dec = (A.mode == BASH_PRG_UNWRAP && ph == 2) ? ~0u : 0u;
        // text: y = the block's output octets, word-aligned to the BLOCK; q = where octet 0 goes.  Dword k of the aligned row
        // qa = q - md holds octets 4 k - md .. 4 k - md + 3: z[k] = y[k] : y[k - 1] shifted by md octets.
        const uint32_t md = (uint32_t)(uintptr_t)q & 3u, fsh = (32u - 8u * md) & 31u, m0 = md ? 0u : ~0u;
        uint8_t *qa = q - md;
        const uint32_t end = md + cnt, kt = end >> 2, tb = end & 3u;             // whole dwords: k < kt (k = 0 only if md = 0)
        uint32_t zt = 0, z0 = 0, ycarry = 0;
        const auto chunk = [&](auto Cc) {
            constexpr uint32_t J0 = 8 * decltype(Cc)::value, J1 = J0 + 8 < NW ? J0 + 8 : NW, N = J1 - J0;
            uint32_t Aw[N + 3], Bw[N + 1], y[N];
#pragma unroll
            for (uint32_t j = 0; j < N + 3; ++j) Aw[j] = __builtin_amdgcn_bitop3_b32(Wq(J0 + j), Wq(J0 + j + 1), m1, 0xD8);    // m1 ? W[j + 1] : W[j]
#pragma unroll
            for (uint32_t j = 0; j <= N; ++j) Bw[j] = __builtin_amdgcn_bitop3_b32(Aw[j], Aw[j + 2], m2, 0xD8);
#pragma unroll
            for (uint32_t j = 0; j < N; ++j) {
                const int32_t rem = (int32_t)cnt - (int32_t)(4u * (J0 + j));    // word j keeps its first `rem` octets
                const uint32_t keep = rem >= 4 ? ~0u : rem <= 0 ? 0u : (1u << (8 * rem)) - 1u;
                const uint32_t x = __builtin_amdgcn_alignbit(Bw[j + 1], Bw[j], sh) & keep;
                const uint32_t old = S(J0 + j);
                y[j] = old ^ x;
                uint32_t nw = y[j] ^ (old & keep & dec);
                asm volatile("" : "+v"(nw));          // the new word exists HERE: left to itself the compiler carries old, keep and y of
                S(J0 + j) = nw;                       // all 42 words down to the commit and spills half of them
            }
            if (ph == 2) {
                constexpr uint32_t K1 = J1 == NW ? NW + 1 : J1;                  // the last chunk also owns dword NW
#pragma unroll
                for (uint32_t k = J0; k < K1; ++k) {
                    const uint32_t hi = k < NW ? y[k - J0] : 0u, lo = k == J0 ? ycarry : y[k - J0 - 1];
                    const uint32_t z = __builtin_amdgcn_bitop3_b32(__builtin_amdgcn_alignbit(hi, lo, fsh), hi, m0, 0xD8);      // md ? hi:lo >> .. : hi
                    if (k == 0) z0 = z;
                    else zt = k == kt ? z : zt;
                    if (k < kt && (k || md == 0)) reinterpret_cast<uint32_t *>(qa)[k] = z;
                }
                ycarry = y[N - 1];
            }
        };
        const auto work = [&](auto Cc, uint32_t q0, uint32_t q1) {               // chunk Cc after requesting quads q0 .. q1 - 1
            for (uint32_t j = q0; j < q1; ++j) ldq(j);
            __builtin_amdgcn_sched_barrier(0);
            chunk(Cc);
            __builtin_amdgcn_sched_barrier(0);
        };
        ldq(0);
        work(std::integral_constant<uint32_t, 0>{}, 1, 3);
        work(std::integral_constant<uint32_t, 1>{}, 3, 5);
        work(std::integral_constant<uint32_t, 2>{}, 5, 7);
        work(std::integral_constant<uint32_t, 3>{}, 7, 9);
        work(std::integral_constant<uint32_t, 4>{}, 9, 11);
        work(std::integral_constant<uint32_t, 5>{}, 11, 12);
        if (ph == 2) {
            if (md || kt == 0) {                                                 // the octets before the first whole dword
#pragma unroll
                for (uint32_t b = 0; b < 4; ++b)
                    if (b >= md && b < end) qa[b] = (uint8_t)(z0 >> (8 * b));
            }
            if (kt && tb) {                                                      // ... and after the last
#pragma unroll
                for (uint32_t b = 0; b < 3; ++b)
                    if (b < tb) qa[4 * kt + b] = (uint8_t)(zt >> (8 * b));
            }
        }
        // commit (bash_prg.c:95-97): the code of the NEXT command at octet pos, 0x80 at octet r
        {
            const uint32_t code = ph == 0 ? 0x09u : (ph == 1 && A.mode != BASH_PRG_HASH) ? 0x0Du : 0x11u;
            const uint32_t pos = ph == 0 ? 1u + 4u * (A.n_ann + A.n_fixed) : cnt;
            const uint32_t cw = last ? code << (8 * (pos & 3u)) : 0u, cj = pos >> 2, bit = last ? 0x80u : 0u, rj = r >> 2;
#pragma unroll
            for (uint32_t j = 0; j < NW; ++j) S(j) ^= j == cj ? cw : 0u;
#pragma unroll
            for (uint32_t j = 16; j <= NW; ++j) S(j) ^= j == rj ? bit : 0u;
        }
        bash_f<BASH_FUSED_ORDER>(a);
        if (last) {
            ++ph;
            if (ph == 1) {
                const uint64_t h0 = hoff ? hoff[i] : 0, h1 = hoff ? hoff[i + 1] : 0;
                p = hdrs + h0; left = (size_t)(h1 - h0);
            } else if (ph == 2 && A.mode != BASH_PRG_HASH) {
                const uint64_t o0 = off[i];
                p = src + o0; q = dst + o0; left = (size_t)(off[i + 1] - o0);
            } else
                break;
        } else {
            p += r; q += r; left -= r;
        }
    }
    // squeeze (bash_prg.c:233-238): out_len <= 64 <= r octets from the head of the state
    uint8_t *t = tags + (size_t)A.out_len * i;
    if (A.mode != BASH_PRG_UNWRAP) {
#pragma unroll
        for (uint32_t b = 0; b < 64; ++b)
            if (b < A.out_len) t[b] = (uint8_t)(S(b / 4) >> (8 * (b & 3)));
        return;
    }
    uint32_t diff = 0;
#pragma unroll
    for (uint32_t b = 0; b < 64; ++b)
        if (b < A.out_len) diff |= (uint32_t)t[b] ^ ((S(b / 4) >> (8 * (b & 3))) & 0xFFu);
#undef S
    codes[i] = diff ? (uint32_t)ERR_BAD_MAC : (uint32_t)ERR_OK;
    if (diff) {                                       // a refused record keeps no plaintext: zeros over its own octets only
        uint8_t *z = dst + off[i];
        size_t len = (size_t)(off[i + 1] - off[i]);
        for (; len && ((uintptr_t)z & 3u); ++z, --len) *z = 0;
        for (; len >= 4; z += 4, len -= 4) *reinterpret_cast<uint32_t *>(z) = 0;
        for (; len; ++z, --len) *z = 0;
    }
}

// record lengths that decide the launch order: the text for prg-ae, the message for prg-hash
err_t launch_prg_ragged(const BashPrgArgs &A, const void *d_anns, const void *d_hdrs, const void *d_hoff, const void *d_src,
                        const void *d_off, const void *d_order, size_t n, void *d_dst, void *d_tags, void *d_codes, hipStream_t st)
{
    if (n == 0) return ERR_OK;
    if (n > 0xffffffffull) return ERR_BAD_INPUT;
    const uint64_t *key_off = (const uint64_t *)(A.mode == BASH_PRG_HASH ? d_hoff : d_off);
    const uint32_t *ord = (const uint32_t *)d_order;
    if (!ord) {
        const err_t code = ragged_launch_order(key_off, n, st, &ord);
        if (code != ERR_OK) return code;
    }
    hipLaunchKernelGGL(bash_prg_ragged_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, A, (const uint8_t *)d_anns,
                       (const uint8_t *)d_hdrs, (const uint64_t *)d_hoff, (const uint8_t *)d_src, (const uint64_t *)d_off, ord, n,
                       (uint8_t *)d_dst, (uint8_t *)d_tags, (uint32_t *)d_codes);
    B2H_TRY(hipGetLastError());
    return ERR_OK;
}

}  // namespace bee2hip
