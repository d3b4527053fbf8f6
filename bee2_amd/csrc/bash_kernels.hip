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
#include "bashf_tile.hpp"
#include "common.hpp"

namespace bee2hip {

static_assert(BashSlots{}.m[6][0] == 0 && BashSlots{}.m[6][13] == 13 && BashSlots{}.m[6][23] == 23,
              "bash word permutation must have order 6");

// The tile body is bashF_tile_body (bashf_tile.hpp).  The template arguments are the coordinates of the r02 / r03 A/B
// (profiles/r02_bashF_variants.txt, profiles/r03_bashF_nt_ab.txt), whose other forms are retired: LOAD 0 = direct load,
// STORE 2 = half-slab store, ORDER = issue order of the S-layer (bash_dev.hpp), MINW = wavefronts per SIMD, FLAGS 3 = issue
// priority 3 for the loads and for the store phase.  A full tile takes the body's fast path (profiles/bashF_phases.txt).
template <int LOAD, int STORE, int ORDER, int MINW, int FLAGS>
__global__ __launch_bounds__(BASHF_WG, MINW)
void bashF_tile_kernel(uint8_t *__restrict__ states, size_t n)
{
    static_assert(LOAD == 0 && STORE == 2 && FLAGS == 3, "the product form");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    BashfNoStamp none;
    bashF_tile_body<ORDER, true>(states, n, smem, none);
}

err_t launch_bashF_batch(void *d_states, size_t n, hipStream_t st)
{
    if (n == 0) return ERR_OK;
    const size_t per_wg = BASHF_WG;           // one state per lane
    const size_t grid = (n + per_wg - 1) / per_wg;
    if (grid > 0x7fffffffull) return ERR_BAD_INPUT;
    // W = 4, priority, direct load, half-slab store (v61 of profiles/r02_bashF_variants.txt)
    hipLaunchKernelGGL((bashF_tile_kernel<0, 2, 124, 6, 3>), dim3((unsigned)grid), dim3(BASHF_WG), BASHF_LDS, st, (uint8_t *)d_states, n);
    B2H_TRY(hipGetLastError());
    return ERR_OK;
}

}  // namespace bee2hip
