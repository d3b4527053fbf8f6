// bash_kernels.hip -- batched bash-f and the lane-per-message bash sponge on gfx950.
//
// bashF_tile_kernel   : H1 of SURVEY.md 8a -- n independent 192-byte states,
//                       one lane per state (replaces n calls of bashF,
//                       include/bee2/crypto/bash.h:136).
//
// HBM layout: states are contiguous 192-byte records, exactly bee2's layout.
// A wavefront owns 64 consecutive states = 12 KiB.  Every lane loads its own record,
// permutes it in registers and writes back through LDS (record stride padded to 208
// bytes), so that the stores are coalesced 1 KiB pieces.  Algorithmic traffic: 384 B/state.
#include "bash_dev.hpp"
#include "common.hpp"

namespace bee2hip {

static_assert(BashSlots{}.m[6][0] == 0 && BashSlots{}.m[6][13] == 13 && BashSlots{}.m[6][23] == 23,
              "bash word permutation must have order 6");

constexpr int BASHF_WG = 256;                 // 4 wavefronts
constexpr int BASHF_REC = 192;                // bytes per state
// The store goes through LDS 32 records at a time; every global store is a fully contiguous 1 KiB per
// wave-instruction.  Stride 208 B = 52 dwords keeps the per-lane ds_write_b128 of a whole record bank-conflict free.
constexpr int BASHF_PAD = 208;

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
// One 64-record tile per wavefront: every lane loads its own record directly (16-byte pieces at stride 192),
// the rounds run in registers, and the results go back through a half slab of 32 padded records in two passes
// (6.5 KiB per wavefront) so that every global store is a contiguous 1 KiB.  The template arguments are the
// coordinates of the r02 / r03 A/B (profiles/r02_bashF_variants.txt, profiles/r03_bashF_nt_ab.txt), whose
// other forms are retired: LOAD 0 = direct load, STORE 2 = half-slab store, ORDER = issue order of the S-layer
// (bash_dev.hpp), MINW = wavefronts per SIMD, FLAGS 3 = issue priority 3 for the loads and for the store phase.
template <int LOAD, int STORE, int ORDER, int MINW, int FLAGS>
__global__ __launch_bounds__(BASHF_WG, MINW)
void bashF_tile_kernel(uint8_t *__restrict__ states, size_t n)
{
    static_assert(LOAD == 0 && STORE == 2 && FLAGS == 3, "the product form");
    constexpr int P = STORE, RECS = 64 / P, SLAB = RECS * BASHF_REC;      // SLAB bytes of states per pass
    // the new wavefront is the youngest on its SIMD; without help its address arithmetic and load issue wait behind
    // every older wavefront's VALU work.  Priority 3 until the loads are out.
    __builtin_amdgcn_s_setprio(3);
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint8_t *wl = smem + wave * (RECS * BASHF_PAD);
    const size_t first = ((size_t)blockIdx.x * (BASHF_WG / 64) + wave) * 64;
    if (first >= n) return;
    const size_t left = n - first;
    const int cnt = left < 64 ? (int)left : 64;
    uint8_t *g = states + first * BASHF_REC;
    u64x2 a[24];
    {
        const int r = lane < cnt ? lane : cnt - 1;
        const uint4 *p = reinterpret_cast<const uint4 *>(g + r * BASHF_REC);
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            const uint4 v = p[j];
            a[2 * j].lo = v.x; a[2 * j].hi = v.y; a[2 * j + 1].lo = v.z; a[2 * j + 1].hi = v.w;
        }
    }

    __builtin_amdgcn_s_setprio(0);
    bash_f<ORDER>(a);
    __builtin_amdgcn_s_setprio(3);          // drain the store phase ahead of others' arithmetic

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
    }
}

err_t launch_bashF_batch(void *d_states, size_t n, hipStream_t st)
{
    if (n == 0) return ERR_OK;
    const size_t per_wg = BASHF_WG;           // one state per lane
    const size_t grid = (n + per_wg - 1) / per_wg;
    if (grid > 0x7fffffffull) return ERR_BAD_INPUT;
    // W = 4, priority, direct load, half-slab store (v61 of profiles/r02_bashF_variants.txt)
    constexpr int lds = 4 * 32 * BASHF_PAD;
    hipLaunchKernelGGL((bashF_tile_kernel<0, 2, 124, 6, 3>), dim3((unsigned)grid), dim3(BASHF_WG), lds, st, (uint8_t *)d_states, n);
    B2H_TRY(hipGetLastError());
    return ERR_OK;
}

}  // namespace bee2hip
