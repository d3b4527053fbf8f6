// bashf_tile.hpp -- the body of bashF_tile_kernel (bash_kernels.hip): one 64-record tile per wavefront.
//
// A header of its own so that the phase probe (tools/probe/bashf_phases.hip, not part of libbee2hip.so) can instantiate the
// very same body with time stamps; in the product kernel STAMP = BashfNoStamp and no stamp executes.
#pragma once
#include "bash_dev.hpp"

namespace bee2hip {

constexpr int BASHF_WG = 256;                 // 4 wavefronts
constexpr int BASHF_REC = 192;                // bytes per state
// The store goes through LDS 32 records at a time; every global store is a fully contiguous 1 KiB per
// wave-instruction.  Stride 208 B = 52 dwords keeps the per-lane ds_write_b128 of a whole record bank-conflict free.
constexpr int BASHF_PAD = 208;
constexpr int BASHF_LDS = (BASHF_WG / 64) * 32 * BASHF_PAD;    // a half slab of 32 padded records per wavefront

// Ordering of one wavefront's own LDS traffic.  A workgroup-scope release fence also waits for the
// wavefront's outstanding *global* stores (vmcnt(0)) -- in a walking wavefront that exposed the store
// latency of every tile (r02: 171 us instead of 118), and at the end of a one-tile kernel it keeps the
// slab allocated until the stores are acknowledged.  DS operations of one wavefront execute in order,
// so all that is needed is that the compiler keeps the order and that returned data has arrived.
__device__ __forceinline__ void bashF_wave_sync()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// the stamps of the phase probe: 0 entry, 1 loads issued, 2 loaded data there, 3 end of the rounds, 4 / 5 end of the
// first / second half-slab pass (5 = last store issued)
struct BashfNoStamp {
    template <int I> __device__ __forceinline__ void mark() {}
    __device__ __forceinline__ void wait_loads() {}
};

// a + (b << S) in one full-rate instruction: written out, the compiler folds the small constant products of the
// address arithmetic back into v_mul_u32_u24 (half rate, on the unit the round stream of the other wavefronts needs)
template <int S>
__device__ __forceinline__ uint32_t bashF_lshl_add(uint32_t b, uint32_t a)
{
    uint32_t d;
    asm("v_lshl_add_u32 %0, %1, %2, %3" : "=v"(d) : "v"(b), "n"(S), "v"(a));
    return d;
}

// One 64-record tile per wavefront: every lane loads its own record directly (16-byte pieces at stride 192),
// the rounds run in registers, and the results go back through a half slab of 32 padded records in two passes
// (6.5 KiB per wavefront) so that every global store is a contiguous 1 KiB.
//
// FAST adds one wave-uniform branch on a full tile (cnt == 64: every tile of a batch of a multiple of 64 states):
//   load  : no lane clamp, one base and immediate offsets;
//   store : piece k of a pass is slab bytes [1024 k, 1024 k + 1024) of 32 records at stride 208, i.e. lane l reads
//           o + 16 (o / 192) with o = 1024 k + 16 l.  With q = l / 12, r = l % 12: (64 k + l) / 12 = 5 k + q + carry(4 k + r),
//           and the carry is [r >= 8], [r >= 4], 1, 1 + [r >= 8], 1 + [r >= 4] for k = 1 .. 5 -- three address registers
//           and constant offsets, no exec branch and no multiply per piece; the six reads of a pass go out back to back
//           and each store follows its own data (counted lgkmcnt), the second fill follows the reads, not the stores.
//           Issue priority 3 only while memory instructions are issued, 0 across the full waits.
// Without FAST, and on a partial tile, the general path: per-piece bounds, clamped loads.
template <int ORDER, bool FAST, class STAMP>
__device__ __forceinline__ void bashF_tile_body(uint8_t *__restrict__ states, size_t n, uint8_t *smem, STAMP &stamp)
{
    constexpr int P = 2, RECS = 64 / P, SLAB = RECS * BASHF_REC;          // SLAB bytes of states per pass
    // the new wavefront is the youngest on its SIMD; without help its address arithmetic and load issue wait behind
    // every older wavefront's VALU work.  Priority 3 until the loads are out.
    __builtin_amdgcn_s_setprio(3);
    stamp.template mark<0>();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint8_t *wl = smem + wave * (RECS * BASHF_PAD);
    const size_t first = ((size_t)blockIdx.x * (BASHF_WG / 64) + wave) * 64;
    if (first >= n) return;
    const size_t left = n - first;
    const int cnt = left < 64 ? (int)left : 64;
    const bool full = FAST && cnt == 64;                                  // wave-uniform
    uint8_t *g = states + first * BASHF_REC;
    u64x2 a[24];
    uint32_t mine;                                                        // byte offset of the lane's record in the tile
    if (full) mine = bashF_lshl_add<6>((uint32_t)lane, (uint32_t)lane << 7);      // 192 lane
    else      mine = (uint32_t)((lane < cnt ? lane : cnt - 1) * BASHF_REC);
    {
        const uint4 *p = reinterpret_cast<const uint4 *>(g + mine);
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            const uint4 v = p[j];
            a[2 * j].lo = v.x; a[2 * j].hi = v.y; a[2 * j + 1].lo = v.z; a[2 * j + 1].hi = v.w;
        }
    }
    stamp.template mark<1>();
    stamp.wait_loads();
    stamp.template mark<2>();

    __builtin_amdgcn_s_setprio(0);
    bash_f<ORDER>(a);
    stamp.template mark<3>();
    __builtin_amdgcn_s_setprio(3);          // drain the store phase ahead of others' arithmetic

    if (full) {
        const uint32_t l = (uint32_t)lane, l32 = l & 31u;
        const uint32_t m = l >> 2, q = bashF_lshl_add<1>(m, bashF_lshl_add<3>(m, m)) >> 5;           // l / 12 = (l / 4) 11 / 32
        const uint32_t r = l - (bashF_lshl_add<1>(q, q) << 2);                                      // l % 12
        uint8_t *wr = wl + bashF_lshl_add<4>(l32, bashF_lshl_add<6>(l32, l32 << 7));                 // 208 (l % 32)
        const uint8_t *b0 = wl + ((l + q) << 4);
        const uint8_t *b8 = b0 + (r >= 8 ? 16 : 0), *b4 = b0 + (r >= 4 ? 16 : 0);
        // the twelve 1 KiB pieces of the tile: three wave-uniform bases 4 KiB apart, one lane offset, immediates below 4 KiB
        uint32_t kib4 = 4096;
        asm("" : "+s"(kib4));                                             // opaque: the bases stay scalar, the lane offset stays one register
        uint8_t *g0 = g, *g1 = g0 + kib4, *g2 = g1 + kib4;
        const uint32_t gl = l << 4;
#pragma unroll
        for (int h = 0; h < P; ++h) {
            if ((lane >> 5) == h) {
#pragma unroll
                for (int j = 0; j < 12; ++j) {
                    uint4 v;
                    v.x = a[2 * j].lo; v.y = a[2 * j].hi; v.z = a[2 * j + 1].lo; v.w = a[2 * j + 1].hi;
                    *reinterpret_cast<uint4 *>(wr + 16 * j) = v;
                }
            }
            __builtin_amdgcn_s_setprio(0);
            bashF_wave_sync();
            __builtin_amdgcn_s_setprio(3);
            const uint4 d0 = *reinterpret_cast<const uint4 *>(b0);
            __builtin_amdgcn_sched_barrier(0);
            const uint4 d1 = *reinterpret_cast<const uint4 *>(b8 + (1024 + 80));
            __builtin_amdgcn_sched_barrier(0);
            const uint4 d2 = *reinterpret_cast<const uint4 *>(b4 + (2048 + 160));
            __builtin_amdgcn_sched_barrier(0);
            const uint4 d3 = *reinterpret_cast<const uint4 *>(b0 + (3072 + 240 + 16));
            __builtin_amdgcn_sched_barrier(0);
            const uint4 d4 = *reinterpret_cast<const uint4 *>(b8 + (4096 + 320 + 16));
            __builtin_amdgcn_sched_barrier(0);
            const uint4 d5 = *reinterpret_cast<const uint4 *>(b4 + (5120 + 400 + 16));
            __builtin_amdgcn_sched_barrier(0);                            // the six reads out in this order before the first store waits
            if (h == 0) {
                *reinterpret_cast<uint4 *>(g0 + gl) = d0;
                *reinterpret_cast<uint4 *>(g0 + gl + 1024) = d1;
                *reinterpret_cast<uint4 *>(g0 + gl + 2048) = d2;
                *reinterpret_cast<uint4 *>(g0 + gl + 3072) = d3;
                *reinterpret_cast<uint4 *>(g1 + gl) = d4;
                *reinterpret_cast<uint4 *>(g1 + gl + 1024) = d5;
            } else {
                *reinterpret_cast<uint4 *>(g1 + gl + 2048) = d0;
                *reinterpret_cast<uint4 *>(g1 + gl + 3072) = d1;
                *reinterpret_cast<uint4 *>(g2 + gl) = d2;
                *reinterpret_cast<uint4 *>(g2 + gl + 1024) = d3;
                *reinterpret_cast<uint4 *>(g2 + gl + 2048) = d4;
                *reinterpret_cast<uint4 *>(g2 + gl + 3072) = d5;
            }
            if (h == 0) stamp.template mark<4>();
        }
        stamp.template mark<5>();
        return;
    }

#pragma unroll
    for (int h = 0; h < P; ++h) {
        bashF_wave_sync();
        if (lane / RECS == h && lane < cnt) {
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                uint4 v;
                v.x = a[2 * j].lo; v.y = a[2 * j].hi; v.z = a[2 * j + 1].lo; v.w = a[2 * j + 1].hi;
                *reinterpret_cast<uint4 *>(wl + (lane % RECS) * BASHF_PAD + 16 * j) = v;
            }
        }
        bashF_wave_sync();
        const int bytes = cnt * BASHF_REC - h * SLAB;
#pragma unroll
        for (int k = 0; k < SLAB / 1024; ++k) {
            const int o = k * 1024 + lane * 16;
            if (o < bytes) {
                const int rec = o / BASHF_REC, off = o % BASHF_REC;
                const uint4 v = *reinterpret_cast<const uint4 *>(wl + rec * BASHF_PAD + off);
                *reinterpret_cast<uint4 *>(g + h * SLAB + o) = v;
            }
        }
        if (h == 0) stamp.template mark<4>();
    }
    stamp.template mark<5>();
}

}  // namespace bee2hip
