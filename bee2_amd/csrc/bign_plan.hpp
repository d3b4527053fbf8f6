// bign_plan.hpp -- which kernels a bign batch runs, decided from the batch size, the curve (N = l / 16 32-bit words: 8 / 12 / 16) and
// the tests' overrides, and nothing else: pure functions without HIP (tests/hostshim/bign_plan_main.cpp holds them to the decision
// table on the CPU).  The launchers of bign_kernels.hip and bign_sign_kernels.hip ask once and launch what the plan says; every
// threshold lives here, with the measurement that put it there.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace bee2hip {

constexpr size_t bign_pow2(int e) { return (size_t)1 << e; }

// What tests and A/B runs force (bee2hip_internal_tune 2: verify_path + 16 x verify_lanes, 22: onekey_quads, 10: sign_lanes); the
// defaults decide by batch size.  The values are told where they are read, below.
struct BignForce {
    int verify_path = 0, verify_lanes = 0, onekey_quads = -1, sign_lanes = 0;
    void set_verify(int v) { verify_path = v & 15; verify_lanes = v >> 4; }   // 0x43: quads at every size
};

// ---- verification: slow kernel -> shared inversion -> hash tail (every launcher ends with these) -----------------------------------
struct FinishPlan { size_t k_inv, inv_lanes; bool tail_wide; };   // signatures per inversion; lanes of bign_inv_kernel; 1024- / 64-lane tail
inline FinishPlan finish_plan(int N, size_t n)
{
    // signatures per inversion.  Each lane runs one chain (division steps, then 5 multiplications per
    // signature) and a lone wavefront issues at about a third of a SIMD's rate, so fewer, longer lanes cost
    // little until the lanes no longer cover the SIMDs: measured best at 2^18 signatures K = 8 on the 256-bit
    // curve (72 us; K = 2: 105 us) and K = 4 on the wider ones (profiles/r01_bign_ab_inv.txt)
    // (round 4: with the division-step inversion the optimum is flat; up to 2^17 signatures on the 256-bit curve 2^16
    //  lanes -- one wavefront per SIMD, two signatures each -- are 4-7 % ahead of 2^15; profiles/r04_inv_lanes_ab.txt)
    const size_t want = N == 8 && n > bign_pow2(17) ? 32768 : 65536;
    const size_t k_inv = std::min<size_t>(16, std::max<size_t>(1, n / want));
    return {k_inv, (n + k_inv - 1) / k_inv, N == 8 && n >= 65536};
}

// ---- general verification ----------------------------------------------------------------------------------------------------------
enum class Walk { QUAD, LANE29, LANE32 };
struct VerifyPlan {
    Walk walk;                  // who walks the scalar multiplication: bign_quad29_kernel | prep + bign_main29_kernel | prep + bign_main_kernel
    int wg, lanes;              // QUAD: lanes per block and per signature (2 a pair, 4 a quad, 8 a quad and its helper quad)
    bool points;                // lane forms: the first half of prep is a kernel of its own (the wider curves)
    int sp;                     //   signatures per lane in prep (shared inversion)
    int main29_wg;              //   LANE29: lanes per block
    bool pair_main;             //   LANE32: VtOpsP
    FinishPlan fin;
};
constexpr size_t VERIFY_QUAD_MAX = bign_pow2(15);     // lanes-per-signature forms up to here, one lane per signature above (every curve)
inline VerifyPlan verify_plan(int N, size_t n, const BignForce &f)
{
    VerifyPlan P{};
    P.fin = finish_plan(N, n);
    // Which kernels walk the scalar multiplication (verify_path: 0 by size, 1 always the 32-bit
    // kernels, 2 the 29-bit main kernel, 3 the quad / pair kernel, + 16 x lanes to force quads (0x43), pairs (0x23) or quads with a helper quad (0x83; 0x93 / 0xA3 with 64 / 256 lanes per block)
    // -- tests and A/B):
    //   <= 2^14 signatures: one signature per quad, 29-bit limbs (prep + main in one kernel, no table inversion)
    //   <= 2^15           : one signature per pair of lanes, same kernel (256-bit curve; the wider ones use quads up
    //                       to 2^15 and the 32-bit kernels above: 28- / 27-bit limbs, LZ<N>)
    //   <= 2^18           : one lane per signature, 29-bit limbs, the multiplication one asm block (bign_fe29_asm.inc; round 6: it
    //                       beats the 32-bit kernels at four wavefronts per SIMD too: 1 662 against 1 768 us at 2^18)
    //   above             : one lane per signature, 32-bit limbs (the throughput form)
    int path = 1;
    if (N == 8) path = f.verify_path ? f.verify_path : n <= VERIFY_QUAD_MAX ? 3 : n <= bign_pow2(18) ? 2 : 1;   // (round 6: the 29-bit kernel's multiplication is one asm block now -- it beats the 32-bit kernels up to 2^18: profiles/r06_f29_asm_ab.txt)
    // wider curves, quads only: up to 2^14 signatures they leave one wavefront per SIMD; up to 2^15 two, which costs twice
    // the time (2.4 / 4.7 ms) and still beats the one-lane kernels' latency floor (3.4 / 6.7 ms, profiles/r03_verify_wide.txt)
    else path = f.verify_path == 1 || f.verify_path == 3 ? f.verify_path : n <= VERIFY_QUAD_MAX ? 3 : 1;
    if (path == 3) {
        P.walk = Walk::QUAD;
        P.wg = 256;
        P.lanes = 4;
        if (N == 8) P.lanes = f.verify_lanes == 2 ? 2 : f.verify_lanes ? 4 : n <= bign_pow2(14) ? 4 : 2;
        if (P.lanes == 2) return P;
        // up to 2^13 signatures a helper quad per signature takes the comb of u off the main quad's chain (x1.05, x1.10
        // at 2^13).  Four-wave blocks, because wavefronts of a block share a CU's instruction fetches and this
        // kernel is long; around 2^12 one-wave blocks spread over all CUs win (tools/ab/verify_helper_ab.py).
        const bool helper = f.verify_lanes >= 8 || (f.verify_lanes == 0 && n <= bign_pow2(13));
        const bool one_wave = f.verify_lanes == 9 || (f.verify_lanes != 10 && n > 3 * bign_pow2(10) && n <= bign_pow2(12));
        if (helper) P.lanes = 8;                             // (without it: 256 / 4, also what 0x43 forces at every size)
        if (helper && one_wave) P.wg = 64;
        return P;
    }
    P.walk = N == 8 && path == 2 ? Walk::LANE29 : Walk::LANE32;
    P.points = N != 8;
    P.sp = n >= bign_pow2(18) ? 2 : 1;           // signatures per lane in prep (shared inversion)
    // The MAIN kernel takes its multiply-adds in pairs (VtOpsP, bign_dev.hpp mac2) where that pays -- measured,
    // profiles/r04_mad_pairs_vt.txt: the 384- / 512-bit curves up to 2^16 signatures (ONE wavefront per SIMD: 2.85 -> 2.14 ms and
    // 6.26 -> 4.82 ms at 2^16), the 256-bit curve from 2^18 on (four wavefronts: +0.8 % at 2^18, +1.7 % at 2^19); at two wavefronts
    // per SIMD the paired form loses 2-5 % on every curve, and points / prep do not care.
    if (P.walk == Walk::LANE32) P.pair_main = N == 8 ? n >= bign_pow2(18) : n <= bign_pow2(16);
    else P.main29_wg = n <= bign_pow2(14) ? 64 : 256;
    return P;
}

// ---- one signer / a few signers ----------------------------------------------------------------------------------------------------
struct OnekeyPlan { bool quad, q16; FinishPlan fin; };   // four lanes per signature | one; the key's 16-bit table read (one signer only)
inline OnekeyPlan onekey_plan(int N, size_t n, bool keyed, bool has_tab16, const BignForce &f)
{
    // up to 2^16 signatures: four lanes per signature (a third of the latency; at 2^17 the one-lane kernels' two wavefronts per SIMD tie)
    const bool quad = f.onekey_quads > 0 || (f.onekey_quads < 0 && n <= bign_pow2(16));
    return {quad, !keyed && has_tab16, finish_plan(N, n)};
}

// ---- k G of the signing side -------------------------------------------------------------------------------------------------------
// k G by one lane per scalar (throughput) or by 64 / 16 / 4 lanes per scalar (latency; each form fills the device -- one
// wavefront per SIMD -- at 2^10 / 2^12 / 2^14 scalars).  sign_lanes: 0 = by batch size; 1 = one lane (signed 6-bit windows,
// Jacobian mixed additions), 4 / 16 / 64 = that many lanes, 8 = the LDS look-up form (256-bit curve; elsewhere by size) --
// forced by bee2hip_internal_tune 10.  profiles/r03_sign_coop.txt measures the forms at every size on the three curves:
// 64 lanes up to 2^10 scalars, 16 up to 2^13, 4 up to 2^15, one lane above.
// (round 4) 8 = one lane per scalar with the window's entry looked up in LDS (bign_mulbase_lds_kernel: 256-bit curve only,
// signed 8-bit windows and 16 copies of the row): from 3 * 2^16 scalars on, where its one round of <= 256 workgroups (0.63 ms)
// beats the scanning kernel's 256-lane blocks (0.55 ms at 2^17, 0.97 ms at 2^18: profiles/r04_sign_lds.txt)
constexpr size_t MULBASE_LDS_MIN = bign_pow2(15), MULBASE_LDS_512_MAX = bign_pow2(17);   // (512-lane workgroups; round 6: from 2^15 scalars -- the 29-bit form with the shared inversion
//  takes 0.27 | 0.35 ms (key | signature) for anything up to 2^17, the 4-lane cooperative form 0.35 | 0.43 ms at 2^15: profiles/r06_sign_l29_ab.txt)
// lanes: 64 / 16 / 4 = cooperative forms on the 4-bit windows of the seed table; 8 = the LDS look-up form; 1 = one lane per
// scalar, signed 6-bit windows (tab6), Jacobian mixed additions
struct MulbasePlan { int lanes, wg; };                   // wg: form 8 only
inline MulbasePlan mulbase_plan(int N, size_t n, const BignForce &f)
{
    const int s = f.sign_lanes;
    if (s == 1 || s == 4 || s == 16 || s == 64) return {s, 0};
    // up to 2^17 scalars: workgroups of 512 lanes (<= 256 of them: one per CU, two wavefronts per SIMD); above: 1024 lanes
    if (N == 8 && (s == 8 || (s == 0 && n >= MULBASE_LDS_MIN))) return {8, n <= MULBASE_LDS_512_MAX ? 512 : 1024};
    return {n <= bign_pow2(10) ? 64 : n <= bign_pow2(13) ? 16 : n <= bign_pow2(15) ? 4 : 1, 0};
}

// ---- the hashing kernels of signing ------------------------------------------------------------------------------------------------
constexpr int SIGN_WG_MIN = 256;                         // = SIGN_WG, the lanes of a workgroup below 2^17 signatures
constexpr size_t SIGN_TAB_BYTES = 64 * 1024, CU_LDS_BYTES = 160 * 1024;     // = BeltTabTwo::kBytes; what a CU has
// lanes per workgroup (one 64 KiB table each): big batches take the largest that fits the CU's 160 KiB with its rows
// (256-bit curve, no t: 1024 lanes for the nonce, 512 for the tail -- 4 and 2 wavefronts per SIMD where it used to be 1)
inline int sign_wg(size_t n, uint32_t row_words)
{
    // ... as long as every CU still gets a workgroup: 2^16 signatures in 64 workgroups of 1024 lose 8 % (profiles/r03_sign_wg.txt)
    if (n < bign_pow2(17)) return SIGN_WG_MIN;
    const int cap = n < bign_pow2(18) ? 512 : 1024;
    for (int wg = cap; wg > SIGN_WG_MIN; wg >>= 1)
        if (SIGN_TAB_BYTES + (size_t)wg * row_words * 4 <= CU_LDS_BYTES) return wg;
    return SIGN_WG_MIN;
}

}  // namespace bee2hip
