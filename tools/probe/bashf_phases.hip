// bashf_phases.hip -- diagnostic, NOT part of libbee2hip.so: the body of bashF_tile_kernel (bee2_amd/csrc/bashf_tile.hpp) with
// s_memtime stamps at the edges of a wavefront's life: 0 entry, 1 loads issued, 2 loaded data there, 3 end of the rounds,
// 4 end of the first half-slab pass, 5 last store issued.  Wavefront 0 of every stride-th workgroup stamps; its lane 0 writes
// {t0 .. t5, workgroup, 0} as eight u64 to a side buffer.  fast = 0 is the general path on every tile (the kernel before the
// full-tile fast path), fast = 1 the product's body.  Stamps cost wave cycles (about 11 %): read the SHARES, never the run time.
// Built by __graft_entry__.build() into bee2_amd/lib/libb2hphases.so; tools/ab/bashf_phases.py loads it with ctypes.
#include <hip/hip_runtime.h>

#include "../../bee2_amd/csrc/bashf_tile.hpp"

using namespace bee2hip;

struct BashfStamp {
    unsigned long long t[6] = {};
    bool on = false;                          // wave-uniform
    template <int I> __device__ __forceinline__ void mark()
    {
        if (!on) return;
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t[I]) :: "memory");
        __builtin_amdgcn_sched_barrier(0);
    }
    // the rounds' first instruction waits for every load anyway (vmcnt(0) at the head of the round loop)
    __device__ __forceinline__ void wait_loads() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
};

template <bool FAST>
__global__ __launch_bounds__(BASHF_WG, 6)
void bashF_tile_stamped(uint8_t *__restrict__ states, size_t n, unsigned long long *__restrict__ stamps, unsigned stride)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    BashfStamp st;
    st.on = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == 0 && blockIdx.x % stride == 0;
    bashF_tile_body<124, FAST>(states, n, smem, st);
    // the lane from mbcnt: threadIdx.x kept alive to this point costs the body a register it does not have
    if (st.on && __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0) {
        unsigned long long *o = stamps + (size_t)(blockIdx.x / stride) * 8;
#pragma unroll
        for (int i = 0; i < 6; ++i) o[i] = st.t[i];
        o[6] = blockIdx.x;
        o[7] = 0;
    }
}

// d_stamps: stamps_cap u64, at least 8 per stamping workgroup; returns the hipError_t of the launch, -1 on bad arguments
extern "C" __attribute__((visibility("default"))) int b2h_bashf_phases(void *d_states, size_t n, int fast, void *d_stamps,
                                                                       size_t stamps_cap, unsigned stride, void *stream)
{
    if (n == 0 || stride == 0 || !d_states || !d_stamps) return -1;
    const size_t grid = (n + BASHF_WG - 1) / BASHF_WG;
    if (grid > 0x7fffffffull || ((grid + stride - 1) / stride) * 8 > stamps_cap) return -1;
    if (fast)
        hipLaunchKernelGGL(bashF_tile_stamped<true>, dim3((unsigned)grid), dim3(BASHF_WG), BASHF_LDS, (hipStream_t)stream,
                           (uint8_t *)d_states, n, (unsigned long long *)d_stamps, stride);
    else
        hipLaunchKernelGGL(bashF_tile_stamped<false>, dim3((unsigned)grid), dim3(BASHF_WG), BASHF_LDS, (hipStream_t)stream,
                           (uint8_t *)d_states, n, (unsigned long long *)d_stamps, stride);
    return (int)hipGetLastError();
}
