// bign_plan_main.cpp -- bee2_amd/csrc/bign_plan.hpp held to its decision table, without a GPU and without HIP: the header alone and this
// file make the program (tests/test_host_bign_plan.py builds it plain and with ASan + UBSan and runs it as a process).
// The rows below are the table written out: [lo, hi] signatures -> what the plan must say.  Every (curve, override) is asked at
// every size of `sizes()` -- 1, 2, 63, 64, 65, every switch b of the table with b - 1 and b + 1, 2^19, 2^20, 2^24 -- and each answer
// must be covered by exactly one row and equal it; on top of that the invariants a launcher relies on (wg % lanes == 0, the
// inversion lanes cover the batch, the signing workgroup's LDS fits a CU) are checked at every size.
#include <cstdio>
#include <vector>

#include "../../bee2_amd/csrc/bign_plan.hpp"

using namespace bee2hip;

static int g_failed = 0;
#define CHECK(cond, ...)                                                        \
    do {                                                                        \
        if (!(cond)) {                                                          \
            ++g_failed;                                                         \
            std::printf("FAILED %s:%d %s -- ", __FILE__, __LINE__, #cond);       \
            std::printf(__VA_ARGS__);                                           \
            std::printf("\n");                                                  \
        }                                                                       \
    } while (0)

constexpr size_t K = 1024, INF = ~(size_t)0;
constexpr int L128 = 1, L192 = 2, L256 = 4, WIDE = L192 | L256, ALL = L128 | WIDE;
static int level_bit(int l) { return l == 128 ? L128 : l == 192 ? L192 : L256; }

static std::vector<size_t> sizes()
{
    std::vector<size_t> v = {1, 2, 63, 64, 65, 512 * K, 1024 * K, 16384 * K};
    for (size_t b : {1 * K, 3 * K, 4 * K, 8 * K, 16 * K, 32 * K, 64 * K, 128 * K, 256 * K})
        for (size_t n : {b - 1, b, b + 1}) v.push_back(n);
    return v;
}

// ---- general verification: tune key 2 -> rows ------------------------------------------------------------------------------------------
struct VRow {
    int force, levels;          // the value of tune key 2; the curves the row speaks of
    size_t lo, hi;
    Walk walk;
    int wg, lanes;              // QUAD
    int points, sp, main29_wg, pair_main;   // lane forms (main29_wg: LANE29, pair_main: LANE32)
};
constexpr Walk Q = Walk::QUAD, L29 = Walk::LANE29, L32 = Walk::LANE32;
static const VRow k_verify[] = {
    // unforced, l = 128
    {0, L128, 1, 3072, Q, 256, 8},
    {0, L128, 3073, 4096, Q, 64, 8},
    {0, L128, 4097, 8192, Q, 256, 8},
    {0, L128, 8193, 16384, Q, 256, 4},
    {0, L128, 16385, 32768, Q, 256, 2},
    {0, L128, 32769, 262143, L29, 0, 0, 0, 1, 256, 0},
    {0, L128, 262144, 262144, L29, 0, 0, 0, 2, 256, 0},
    {0, L128, 262145, INF, L32, 0, 0, 0, 2, 0, 1},
    // unforced, l = 192 / 256
    {0, WIDE, 1, 3072, Q, 256, 8},
    {0, WIDE, 3073, 4096, Q, 64, 8},
    {0, WIDE, 4097, 8192, Q, 256, 8},
    {0, WIDE, 8193, 32768, Q, 256, 4},
    {0, WIDE, 32769, 65536, L32, 0, 0, 1, 1, 0, 1},
    {0, WIDE, 65537, 262143, L32, 0, 0, 1, 1, 0, 0},
    {0, WIDE, 262144, INF, L32, 0, 0, 1, 2, 0, 0},
    // 1: the 32-bit kernels at every size; pair_main by size
    {1, L128, 1, 262143, L32, 0, 0, 0, 1, 0, 0},
    {1, L128, 262144, INF, L32, 0, 0, 0, 2, 0, 1},
    {1, WIDE, 1, 65536, L32, 0, 0, 1, 1, 0, 1},
    {1, WIDE, 65537, 262143, L32, 0, 0, 1, 1, 0, 0},
    {1, WIDE, 262144, INF, L32, 0, 0, 1, 2, 0, 0},
    // a path nibble that is none of 1, 2, 3 walks as 1 on l = 128
    {4, L128, 1, 262143, L32, 0, 0, 0, 1, 0, 0},
    {4, L128, 262144, INF, L32, 0, 0, 0, 2, 0, 1},
    // 2: the 29-bit main kernel at every size (l = 128); ignored on the wider curves
    {2, L128, 1, 16384, L29, 0, 0, 0, 1, 64, 0},
    {2, L128, 16385, 262143, L29, 0, 0, 0, 1, 256, 0},
    {2, L128, 262144, INF, L29, 0, 0, 0, 2, 256, 0},
    {2, WIDE, 1, 3072, Q, 256, 8},
    {2, WIDE, 3073, 4096, Q, 64, 8},
    {2, WIDE, 4097, 8192, Q, 256, 8},
    {2, WIDE, 8193, 32768, Q, 256, 4},
    {2, WIDE, 32769, 65536, L32, 0, 0, 1, 1, 0, 1},
    {2, WIDE, 65537, 262143, L32, 0, 0, 1, 1, 0, 0},
    {2, WIDE, 262144, INF, L32, 0, 0, 1, 2, 0, 0},
    // 3: quads at every size, lanes / helper / wg by size
    {3, ALL, 1, 3072, Q, 256, 8},
    {3, ALL, 3073, 4096, Q, 64, 8},
    {3, ALL, 4097, 8192, Q, 256, 8},
    {3, L128, 8193, 16384, Q, 256, 4},
    {3, L128, 16385, INF, Q, 256, 2},
    {3, WIDE, 8193, INF, Q, 256, 4},
    // 0x43 quads, 0x23 pairs (quads on the wider curves), 0x83 helper quads (block by size), 0x93 / 0xA3 one-wave / four-wave blocks
    {0x43, ALL, 1, INF, Q, 256, 4},
    {0x23, L128, 1, INF, Q, 256, 2},
    {0x23, WIDE, 1, INF, Q, 256, 4},
    {0x83, ALL, 1, 3072, Q, 256, 8},
    {0x83, ALL, 3073, 4096, Q, 64, 8},
    {0x83, ALL, 4097, INF, Q, 256, 8},
    {0x93, ALL, 1, INF, Q, 64, 8},
    {0xA3, ALL, 1, INF, Q, 256, 8},
};

// ---- the finish: k_inv and the tail ----------------------------------------------------------------------------------------------------
// (the rows cover the sizes of sizes() only, not every n: between them k_inv takes the values in between -- a size added there
//  needs its row, or it reports "0 finish rows")
struct FRow { int levels; size_t lo, hi, k_inv; int tail_wide; };
static const FRow k_finish[] = {
    {L128, 1, 65535, 1, 0},
    {L128, 65536, 131071, 1, 1},
    {L128, 131072, 131072, 2, 1},
    {L128, 131073, 163839, 4, 1},
    {L128, 229376, 262143, 7, 1},
    {L128, 262144, 294911, 8, 1},
    {L128, 524288, INF, 16, 1},
    {WIDE, 1, 131071, 1, 0},
    {WIDE, 131072, 196607, 2, 0},
    {WIDE, 196608, 262143, 3, 0},
    {WIDE, 262144, 327679, 4, 0},
    {WIDE, 524288, 589823, 8, 0},
    {WIDE, 1048576, INF, 16, 0},
};
static void check_finish(int l, size_t n, const FinishPlan &F, const char *who)
{
    int hits = 0;
    for (const FRow &r : k_finish) {
        if (!(r.levels & level_bit(l)) || n < r.lo || n > r.hi) continue;
        ++hits;
        CHECK(F.k_inv == r.k_inv && (int)F.tail_wide == r.tail_wide && F.inv_lanes == (n + r.k_inv - 1) / r.k_inv,
              "%s l=%d n=%zu: k_inv %zu lanes %zu wide %d", who, l, n, F.k_inv, F.inv_lanes, (int)F.tail_wide);
    }
    CHECK(hits == 1, "%s l=%d n=%zu: %d finish rows", who, l, n, hits);
    CHECK(F.k_inv >= 1 && F.k_inv <= 16 && F.inv_lanes * F.k_inv >= n && F.inv_lanes <= n, "%s l=%d n=%zu: k_inv %zu lanes %zu", who, l, n,
          F.k_inv, F.inv_lanes);
}

static void check_verify(int l, int force, size_t n)
{
    BignForce f;
    f.set_verify(force);
    const VerifyPlan P = verify_plan(l / 16, n, f);
    int hits = 0;
    for (const VRow &r : k_verify) {
        if (r.force != force || !(r.levels & level_bit(l)) || n < r.lo || n > r.hi) continue;
        ++hits;
        bool same = P.walk == r.walk;
        if (same && r.walk == Q) same = P.wg == r.wg && P.lanes == r.lanes;
        if (same && r.walk != Q) same = (int)P.points == r.points && P.sp == r.sp;
        if (same && r.walk == L29) same = P.main29_wg == r.main29_wg;
        if (same && r.walk == L32) same = (int)P.pair_main == r.pair_main;
        CHECK(same, "verify l=%d force=0x%x n=%zu: walk %d wg %d lanes %d points %d sp %d main29_wg %d pair_main %d", l, force, n, (int)P.walk,
              P.wg, P.lanes, (int)P.points, P.sp, P.main29_wg, (int)P.pair_main);
    }
    CHECK(hits == 1, "verify l=%d force=0x%x n=%zu: %d rows", l, force, n, hits);
    if (P.walk == Q)
        CHECK((P.lanes == 2 || P.lanes == 4 || P.lanes == 8) && (P.wg == 64 || P.wg == 256) && P.wg % P.lanes == 0 && (P.lanes != 2 || l == 128),
              "verify l=%d force=0x%x n=%zu: wg %d lanes %d", l, force, n, P.wg, P.lanes);
    else
        CHECK((P.sp == 1 || P.sp == 2) && P.points == (l != 128) && (P.walk != L29 || (l == 128 && (P.main29_wg == 64 || P.main29_wg == 256))),
              "verify l=%d force=0x%x n=%zu: sp %d points %d main29_wg %d", l, force, n, P.sp, (int)P.points, P.main29_wg);
    check_finish(l, n, P.fin, "verify");
}

// ---- one signer / keyed ----------------------------------------------------------------------------------------------------------------
struct ORow { int quads; size_t lo, hi; int quad; };      // tune key 22: any value above 0 forces four lanes, any below 0 decides by size
static const ORow k_onekey[] = {
    {-1, 1, 65536, 1}, {-1, 65537, INF, 0}, {-2, 1, 65536, 1}, {-2, 65537, INF, 0},
    {0, 1, INF, 0},
    {1, 1, INF, 1}, {2, 1, INF, 1},
};
static const struct { int keyed, has16, q16; } k_onekey16[] = {{0, 0, 0}, {0, 1, 1}, {1, 0, 0}, {1, 1, 0}};
static void check_onekey(int l, size_t n)
{
    for (int quads : {-2, -1, 0, 1, 2})
        for (const auto &t : k_onekey16) {
            BignForce f;
            f.onekey_quads = quads;
            const OnekeyPlan P = onekey_plan(l / 16, n, t.keyed != 0, t.has16 != 0, f);
            int hits = 0;
            for (const ORow &r : k_onekey) {
                if (r.quads != quads || n < r.lo || n > r.hi) continue;
                ++hits;
                CHECK((int)P.quad == r.quad && (int)P.q16 == t.q16, "onekey l=%d n=%zu quads=%d keyed=%d has16=%d: quad %d q16 %d", l, n, quads,
                      t.keyed, t.has16, (int)P.quad, (int)P.q16);
            }
            CHECK(hits == 1, "onekey l=%d n=%zu quads=%d: %d rows", l, n, quads, hits);
            check_finish(l, n, P.fin, "onekey");
        }
}

// ---- k G of the signing side -----------------------------------------------------------------------------------------------------------
struct MRow { int sign_lanes, levels; size_t lo, hi; int lanes, wg; };
static const MRow k_mulbase[] = {
    {1, ALL, 1, INF, 1, 0}, {4, ALL, 1, INF, 4, 0}, {16, ALL, 1, INF, 16, 0}, {64, ALL, 1, INF, 64, 0},
    {0, L128, 1, 1024, 64, 0},
    {0, L128, 1025, 8192, 16, 0},
    {0, L128, 8193, 32767, 4, 0},
    {0, L128, 32768, 131072, 8, 512},
    {0, L128, 131073, INF, 8, 1024},
    {8, L128, 1, 131072, 8, 512},
    {8, L128, 131073, INF, 8, 1024},
    // by size and never form 8: the wider curves (8 asks in vain there), a value that names no form
    {0, WIDE, 1, 1024, 64, 0}, {0, WIDE, 1025, 8192, 16, 0}, {0, WIDE, 8193, 32768, 4, 0}, {0, WIDE, 32769, INF, 1, 0},
    {8, WIDE, 1, 1024, 64, 0}, {8, WIDE, 1025, 8192, 16, 0}, {8, WIDE, 8193, 32768, 4, 0}, {8, WIDE, 32769, INF, 1, 0},
    {2, ALL, 1, 1024, 64, 0}, {2, ALL, 1025, 8192, 16, 0}, {2, ALL, 8193, 32768, 4, 0}, {2, ALL, 32769, INF, 1, 0},
};
static void check_mulbase(int l, int sign_lanes, size_t n)
{
    BignForce f;
    f.sign_lanes = sign_lanes;
    const MulbasePlan P = mulbase_plan(l / 16, n, f);
    int hits = 0;
    for (const MRow &r : k_mulbase) {
        if (r.sign_lanes != sign_lanes || !(r.levels & level_bit(l)) || n < r.lo || n > r.hi) continue;
        ++hits;
        CHECK(P.lanes == r.lanes && P.wg == r.wg, "mulbase l=%d sign_lanes=%d n=%zu: lanes %d wg %d", l, sign_lanes, n, P.lanes, P.wg);
    }
    CHECK(hits == 1, "mulbase l=%d sign_lanes=%d n=%zu: %d rows", l, sign_lanes, n, hits);
    CHECK(P.lanes != 8 || l == 128, "mulbase l=%d sign_lanes=%d n=%zu: form 8 off the 256-bit curve", l, sign_lanes, n);
}

// ---- sign_wg ---------------------------------------------------------------------------------------------------------------------------
static void check_sign_wg()
{
    // 64 KiB of table leave 96 KiB = 24576 words of rows: 1024 lanes take rows of up to 24 words, 512 lanes of up to 48
    static const struct { uint32_t rw; int wg[4]; } rows[] = {     // n = 2^17 - 1, 2^17, 2^18 - 1, 2^18
        {9, {256, 512, 512, 1024}},  {17, {256, 512, 512, 1024}}, {25, {256, 512, 512, 512}},
        {33, {256, 512, 512, 512}},  {41, {256, 512, 512, 512}},  {49, {256, 256, 256, 256}},
    };
    const size_t at[4] = {128 * K - 1, 128 * K, 256 * K - 1, 256 * K};
    for (const auto &r : rows) {
        for (int i = 0; i < 4; ++i) CHECK(sign_wg(at[i], r.rw) == r.wg[i], "sign_wg(%zu, %u) = %d", at[i], r.rw, sign_wg(at[i], r.rw));
        for (size_t n : sizes()) {
            const int wg = sign_wg(n, r.rw);
            CHECK((wg == 256 || wg == 512 || wg == 1024) && 65536 + (size_t)wg * r.rw * 4 <= 163840 && (n >= 128 * K || wg == 256),
                  "sign_wg(%zu, %u) = %d", n, r.rw, wg);
        }
    }
}

int main()
{
    BignForce d;
    CHECK(d.verify_path == 0 && d.verify_lanes == 0 && d.onekey_quads == -1 && d.sign_lanes == 0, "BignForce's defaults");
    d.set_verify(0xA3);
    CHECK(d.verify_path == 3 && d.verify_lanes == 10, "0xA3 -> path %d lanes %d", d.verify_path, d.verify_lanes);
    for (int l : {128, 192, 256})
        for (size_t n : sizes()) {
            for (int force : {0, 1, 2, 3, 0x43, 0x23, 0x83, 0x93, 0xA3}) check_verify(l, force, n);
            if (l == 128) check_verify(l, 4, n);
            check_onekey(l, n);
            for (int s : {0, 1, 2, 4, 8, 16, 64}) check_mulbase(l, s, n);
        }
    check_sign_wg();
    if (g_failed) { std::printf("bign plan: %d checks failed\n", g_failed); return 1; }
    std::printf("bign plan ok\n");
    return 0;
}
