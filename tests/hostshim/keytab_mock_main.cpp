// TEST INFRASTRUCTURE: the one-signer key-table cache -- bee2_amd/csrc/bign_keytab.hpp -- compiled with g++ against
// tests/hostshim/mockhip (streams = threads, device memory = heap) so that its policy, its locking and its frees run under
// -fsanitize=thread and -fsanitize=address,undefined on a box without a GPU.  The curve is a stand-in: a key is 8 octets, "off the
// curve" when its first octet is 0xEE, and the table "kernel" fills a key's table with a pattern made from the key's octets as they
// arrived in device memory -- so every table a call returns can be checked while it is held: one that was freed too early reads as a
// wrong pattern, and under ASan as a use after free.  Built and run by tests/test_host_keytab.py.  Nothing here ships.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <array>
#include <chrono>
#include <future>
#include <set>
#include "../../bee2_amd/csrc/bign_keytab.hpp"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); fflush(stderr); _Exit(1); } } while (0)

static std::atomic<hipStream_t> g_capturing{nullptr};          // the stream that "is being captured"
static std::atomic<int> g_last_hip{0};
static const char *volatile g_last_what = "";
namespace bee2hip {
bool stream_is_capturing(hipStream_t st) { return st && st == g_capturing.load(); }
err_t hip_fail(hipError_t e, const char *what) { g_last_hip.store(e); g_last_what = what; return ERR_BEE2HIP_DEVICE; }
}  // namespace bee2hip
using namespace bee2hip;
using Tabs = KeyTabCache::Tabs;
using Key = std::array<uint8_t, 8>;

constexpr size_t KEY = 8, BASE = 16, AUX = KEY + BASE, TAB = 64, TAB16 = 128, SLAB4 = 4 * (TAB + AUX);
constexpr uint8_t OFF_CURVE = 0xEE;
static std::atomic<long> g_builds_queued{0};
static std::atomic<mockhip::Latch *> g_block_next_build{nullptr};      // the next table build also parks this latch on g_blocked
static hipStream_t g_blocked = nullptr;

static uint8_t base_at(const uint8_t *key, size_t i) { return (uint8_t)(key[i % KEY] ^ 0x5A ^ (uint8_t)i); }
static uint8_t tab_at(const uint8_t *key, size_t b) { return (uint8_t)(key[b % KEY] * 3 + b + base_at(key, b % BASE)); }
static uint8_t tab16_at(const uint8_t *key, size_t b) { return (uint8_t)(tab_at(key, b % TAB) ^ 0xA5 ^ (uint8_t)(b / TAB)); }

static KeyCurve mock_curve()
{
    KeyCurve c;
    c.id_prefix = {(char)0, (char)8};
    c.key_len = KEY;
    c.tab_bytes = TAB;
    c.aux_bytes = AUX;
    c.tab16_bytes = TAB16;
    c.tab16_log2 = 10;
    c.on_curve_and_base = [](const uint8_t *key, uint8_t *out) {
        if (key[0] == OFF_CURVE) return false;
        for (size_t i = 0; i < BASE; ++i) out[i] = base_at(key, i);
        return true;
    };
    c.queue_build = [](hipStream_t st, const uint8_t *d_aux, uint8_t *d_tabs, size_t M) {
        g_builds_queued.fetch_add(1);
        if (mockhip::Latch *l = g_block_next_build.exchange(nullptr)) mockhipBlock(g_blocked, l);
        mockhipLaunch(st, [=] {                         // (reads what the upload put there: key, then starting points)
            for (size_t j = 0; j < M; ++j)
                for (size_t b = 0; b < TAB; ++b) d_tabs[j * TAB + b] = (uint8_t)(d_aux[j * AUX + b % KEY] * 3 + b + d_aux[j * AUX + KEY + b % BASE]);
        });
    };
    c.queue_build16 = [](hipStream_t st, const void *tab, void *t16) {
        mockhipLaunch(st, [=] { for (size_t b = 0; b < TAB16; ++b) ((uint8_t *)t16)[b] = (uint8_t)(((const uint8_t *)tab)[b % TAB] ^ 0xA5 ^ (uint8_t)(b / TAB)); });
    };
    return c;
}
static const KeyCurve C = mock_curve();

static Key K(unsigned tag) { return Key{(uint8_t)tag, (uint8_t)(tag >> 8), 0x11, 0x22, 0x33, (uint8_t)(tag * 7), 0x55, 0x66}; }
static Key off_curve(unsigned tag) { Key k = K(tag); k[1] = k[0]; k[0] = OFF_CURVE; return k; }
static std::vector<uint8_t> cat(const std::vector<Key> &ks)
{
    std::vector<uint8_t> v;
    for (const Key &k : ks) v.insert(v.end(), k.begin(), k.end());
    return v;
}
static long blocks() { return mockhip::g().live_device_blocks.load(); }

// the tables of `ks`; the call must succeed
static Tabs get(KeyTabCache &cache, const std::vector<Key> &ks, uint64_t credit = 1, bool want16 = true, hipStream_t st = nullptr)
{
    Tabs out;
    const std::vector<uint8_t> keys = cat(ks);
    CHECK(cache.tables(C, out, keys.data(), ks.size(), credit, want16, st) == ERR_OK);
    CHECK(out.size() == ks.size());
    return out;
}
// what a launcher's kernels would read, read now: the 8-bit table, the key in device memory and the 16-bit table if there is one
static bool intact(KeyTabCache &cache, const std::shared_ptr<KeyTab> &t, const Key &key)
{
    const void *tab = nullptr, *tab16 = nullptr;
    cache.view(Tabs{t}, &tab, &tab16);
    if (!tab || tab != t->tab || memcmp(t->d_key, key.data(), KEY)) return false;
    for (size_t b = 0; b < TAB; ++b) if (((const uint8_t *)tab)[b] != tab_at(key.data(), b)) return false;
    for (size_t b = 0; tab16 && b < TAB16; ++b) if (((const uint8_t *)tab16)[b] != tab16_at(key.data(), b)) return false;
    return true;
}
static bool has16(KeyTabCache &cache, const std::shared_ptr<KeyTab> &t)
{
    const void *tab = nullptr, *tab16 = nullptr;
    cache.view(Tabs{t}, &tab, &tab16);
    return tab16 != nullptr;
}
static void small(KeyTabCache &cache)
{
    cache.slots = 4;
    cache.slab_keys = 4;
    cache.bytes_max = 3 * SLAB4;
    cache.tab16_max = 2;
}
// is the key in the cache?  (a look-up that builds nothing; the answer costs the key a stamp)
static bool cached(KeyTabCache &cache, const Key &k)
{
    const unsigned long long b0 = cache.n.builds.load();
    get(cache, {k}, 0, false);
    return cache.n.builds.load() == b0;
}

// ---- a hit: stamp, credit, promotion and its limits ---------------------------------------------------------------------
static void hit(hipStream_t st, hipStream_t cap)
{
    const long base = blocks();
    {
        KeyTabCache cache;
        small(cache);
        Tabs a = get(cache, {K(1)}, 5, true, st);
        CHECK(a[0] && cache.n.builds.load() == 1 && a[0]->used == 5 && intact(cache, a[0], K(1)));
        const uint64_t s1 = a[0]->stamp;
        Tabs b = get(cache, {K(1)}, 7, true, st);
        CHECK(b[0] == a[0] && cache.n.builds.load() == 1 && b[0]->used == 12 && b[0]->stamp > s1);
        // a captured call refreshes the stamp, credits nothing and promotes nothing, however busy the key is
        const uint64_t s2 = b[0]->stamp;
        g_capturing.store(cap);
        Tabs c = get(cache, {K(1)}, 100000, true, cap);
        CHECK(c[0] == a[0] && c[0]->used == 12 && c[0]->stamp > s2 && !has16(cache, c[0]));
        g_capturing.store(nullptr);
        // promotion has to be asked for ...
        get(cache, {K(1)}, 2000, false, st);
        CHECK(a[0]->used == 2012 && !has16(cache, a[0]) && cache.n.tab16_live.load() == 0);
        g_capturing.store(cap);
        get(cache, {K(1)}, 1, true, cap);                // (busy by now, and still not inside a capture)
        CHECK(!has16(cache, a[0]) && blocks() == base + 1);
        g_capturing.store(nullptr);
        get(cache, {K(1)}, 0, true, st);
        CHECK(has16(cache, a[0]) && cache.n.tab16_live.load() == 1 && intact(cache, a[0], K(1)) && blocks() == base + 2);
        // ... and below the line nothing happens
        Tabs d = get(cache, {K(2)}, 1023, true, st);
        CHECK(!has16(cache, d[0]));
        d = get(cache, {K(2)}, 1, true, st);
        CHECK(has16(cache, d[0]) && cache.n.tab16_live.load() == 2 && intact(cache, d[0], K(2)));
        // the limit: a third busy key stays on its 8-bit table
        Tabs e = get(cache, {K(3)}, 5000, true, st);
        CHECK(e[0] && !has16(cache, e[0]) && cache.n.tab16_live.load() == 2 && intact(cache, e[0], K(3)));
        // a 16-bit table goes with its key
        a.clear(); b.clear(); c.clear();
        get(cache, {K(4)}, 1, true, st);
        get(cache, {K(5)}, 1, true, st);                 // (K(1) had the oldest stamp of four)
        CHECK(cache.n.tab16_live.load() == 1);
        e = get(cache, {K(3)}, 0, true, st);
        CHECK(has16(cache, e[0]) && cache.n.tab16_live.load() == 2);
    }
    CHECK(blocks() == base);
    {   // a refused 16-bit allocation is not an error: the key stays on 8 bits, and is promoted by a later call
        KeyTabCache cache;
        small(cache);
        Tabs a = get(cache, {K(1)}, 1, true, st);
        mockhip::g().malloc_fail_in.store(1);
        a = get(cache, {K(1)}, 5000, true, st);
        CHECK(a[0] && !has16(cache, a[0]) && cache.n.tab16_live.load() == 0 && intact(cache, a[0], K(1)));
        mockhip::g().malloc_fail_in.store(2);            // (a new key: the slab is allocated, the 16-bit table refused)
        Tabs b = get(cache, {K(2)}, 5000, true, st);
        CHECK(b[0] && !has16(cache, b[0]) && cache.n.tab16_live.load() == 0 && intact(cache, b[0], K(2)));
        a = get(cache, {K(1)}, 0, true, st);
        CHECK(has16(cache, a[0]) && cache.n.tab16_live.load() == 1 && intact(cache, a[0], K(1)));
    }
    CHECK(blocks() == base);
}

// ---- a miss under capture: an error, and nothing allocated, nothing on the stream -----------------------------------------
static void miss_under_capture(hipStream_t st, hipStream_t cap)
{
    const long base = blocks();
    KeyTabCache cache;
    small(cache);
    Tabs a = get(cache, {K(1)}, 1, true, st);
    const uint64_t s1 = a[0]->stamp;
    mockhip::Global &G = mockhip::g();
    const long b0 = blocks(), c0 = G.async_copies.load(), y0 = G.stream_syncs.load(), q0 = g_builds_queued.load();
    const unsigned long long n0 = cache.n.builds.load();
    g_capturing.store(cap);
    Tabs out;
    const std::vector<uint8_t> keys = cat({K(1), K(2)});
    CHECK(cache.tables(C, out, keys.data(), 2, 1, true, cap) == ERR_BEE2HIP_DEVICE);
    g_capturing.store(nullptr);
    CHECK(g_last_hip.load() == hipErrorStreamCaptureUnsupported);
    CHECK(!strcmp(g_last_what, "key-table miss under stream capture: verify once under each key before capturing"));
    CHECK(blocks() == b0 && G.async_copies.load() == c0 && G.stream_syncs.load() == y0 && g_builds_queued.load() == q0 && cache.n.builds.load() == n0);
    CHECK(a[0]->stamp > s1 && a[0]->used == 1);         // (the hit in front of the miss kept its stamp)
    a.clear(); out.clear();
    (void)base;
}

// ---- misses: built once, together, in slabs; keys off the curve; the 16-bit table at once for a busy newcomer -------------
static void miss(hipStream_t st)
{
    const long base = blocks();
    {
        KeyTabCache cache;
        small(cache);
        cache.slots = 100;
        cache.bytes_max = 100 * SLAB4;
        std::vector<Key> ks;
        for (unsigned i = 0; i < 10; ++i) ks.push_back(K(10 + i));
        ks.insert(ks.begin() + 3, off_curve(1));
        ks.insert(ks.begin() + 6, K(11));                // K(11) twice
        ks.push_back(off_curve(1));                     // and the bad key twice
        mockhip::Global &G = mockhip::g();
        const long c0 = G.async_copies.load(), y0 = G.stream_syncs.load(), q0 = g_builds_queued.load();
        Tabs out = get(cache, ks, 7, true, st);
        CHECK(cache.n.builds.load() == 10);
        CHECK(blocks() == base + 3 && cache.n.slab_bytes.load() == 10 * (TAB + AUX));        // 4 + 4 + 2 keys
        CHECK(G.async_copies.load() == c0 + 3 && g_builds_queued.load() == q0 + 3 && G.stream_syncs.load() == y0 + 3);
        std::set<const KeySlab *> slabs;
        for (size_t k = 0; k < ks.size(); ++k) {
            if (ks[k][0] == OFF_CURVE) { CHECK(!out[k]); continue; }
            CHECK(out[k] && intact(cache, out[k], ks[k]) && out[k]->used == 7 && !has16(cache, out[k]));
            slabs.insert(out[k]->slab.get());
        }
        CHECK(slabs.size() == 3 && out[6] == out[1] && ks[6] == ks[1]);
        Tabs z = get(cache, {K(99)}, 1024, true, st);   // busy on arrival
        CHECK(z[0] && z[0]->used == 1024 && has16(cache, z[0]) && intact(cache, z[0], K(99)) && cache.n.tab16_live.load() == 1);
        Tabs none = get(cache, {off_curve(2)}, 1, true, st);
        CHECK(!none[0] && cache.n.builds.load() == 11);
    }
    CHECK(blocks() == base);
}

// ---- the slot bound: the oldest stamp leaves, its holder keeps a valid table ------------------------------------------------
static void slot_bound(hipStream_t st)
{
    const long base = blocks();
    {
        KeyTabCache cache;
        small(cache);
        Tabs held = get(cache, {K(1), K(2), K(3), K(4)}, 1, true, st);
        get(cache, {K(2)}, 1, true, st);                 // K(2) is the most recent now, K(1) the oldest
        get(cache, {K(5)}, 1, true, st);
        CHECK(intact(cache, held[0], K(1)));            // gone from the cache, valid in its holder's hands
        const unsigned long long n0 = cache.n.builds.load();
        get(cache, {K(2), K(3), K(4), K(5)}, 1, true, st);
        CHECK(cache.n.builds.load() == n0);
        get(cache, {K(1)}, 1, true, st);                 // K(1) again: built again, and K(2) -- the first of the four hits, the oldest now -- leaves
        CHECK(cache.n.builds.load() == n0 + 1 && intact(cache, held[0], K(1)) && intact(cache, held[1], K(2)));
        CHECK(cached(cache, K(3)) && cached(cache, K(4)) && cached(cache, K(5)) && !cached(cache, K(2)));
    }
    CHECK(blocks() == base);
}

// ---- drop_all: every entry leaves, the 16-bit tables with them; a holder keeps a valid table; the keys are built again -------
static void drop_all(hipStream_t st)
{
    const long base = blocks();
    {
        KeyTabCache cache;
        small(cache);
        cache.slots = 100;
        Tabs held = get(cache, {K(1), K(2)}, 1024, true, st);          // busy on arrival: both have their 16-bit table
        get(cache, {K(3), K(4), K(5)}, 1, true, st);
        CHECK(cache.n.tab16_live.load() == 2);
        held.resize(1);
        cache.drop_all();
        CHECK(cache.n.tab16_live.load() == 1 && intact(cache, held[0], K(1)) && has16(cache, held[0]));
        held.clear();
        CHECK(cache.n.tab16_live.load() == 0 && cache.n.slab_bytes.load() == 0 && blocks() == base);
        const unsigned long long n0 = cache.n.builds.load();
        CHECK(!cached(cache, K(1)) && !cached(cache, K(5)) && cache.n.builds.load() == n0 + 2);
        cache.drop_all();
        cache.drop_all();                                               // (empty: nothing to do)
    }
    CHECK(blocks() == base);
}

// ---- the byte bound: idle slabs leave, the one used longest ago first; nothing idle, nothing leaves -------------------------
static void byte_bound(hipStream_t st)
{
    const long base = blocks();
    {
        KeyTabCache cache;
        small(cache);
        cache.slots = 100;
        const auto four = [](unsigned t) { return std::vector<Key>{K(t), K(t + 1), K(t + 2), K(t + 3)}; };
        get(cache, four(10), 1, true, st);
        get(cache, four(20), 1, true, st);
        get(cache, four(30), 1, true, st);
        CHECK(cache.n.slab_bytes.load() == 3 * SLAB4 && blocks() == base + 3);
        get(cache, {K(11)}, 1, true, st);                // slab 10 was used last: slab 20 is the one used longest ago
        Tabs d = get(cache, four(40), 1, true, st);
        d.clear();
        CHECK(cache.n.slab_bytes.load() == 3 * SLAB4 && blocks() == base + 3);
        CHECK(cached(cache, K(30)) && cached(cache, K(43)) && cached(cache, K(10)) && cached(cache, K(13)));
        const unsigned long long n0 = cache.n.builds.load();
        CHECK(!cached(cache, K(20)) && cache.n.builds.load() == n0 + 1);       // (slab 20 left, whole; K(20) back costs a slab: 30 leaves)
        CHECK(cache.n.slab_bytes.load() == 2 * SLAB4 + (TAB + AUX) && !cached(cache, K(21)));
        // every slab has a holder: no idle slab is left, the loop stops, the new slab is allocated past the bound
        Tabs h1 = get(cache, {K(10)}, 1, true, st), h2 = get(cache, {K(40)}, 1, true, st), h3 = get(cache, {K(20)}, 1, true, st), h4 = get(cache, {K(21)}, 1, true, st);
        const size_t before = cache.n.slab_bytes.load();
        const long blocks_before = blocks();
        Tabs e = get(cache, four(50), 1, true, st);
        CHECK(cache.n.slab_bytes.load() == before + SLAB4 && cache.n.slab_bytes.load() > cache.bytes_max && blocks() == blocks_before + 1);
        for (unsigned i = 0; i < 4; ++i) CHECK(e[i] && intact(cache, e[i], K(50 + i)));
        CHECK(intact(cache, h1[0], K(10)) && intact(cache, h2[0], K(40)) && intact(cache, h3[0], K(20)) && intact(cache, h4[0], K(21)));
    }
    CHECK(blocks() == base);
}

// ---- a slab whose tables left one by one while a caller holds one of them is not idle: its bytes are not counted as freed -------
static void slab_with_a_holder_outside(hipStream_t st)
{
    const long base = blocks();
    {
        KeyTabCache cache;
        small(cache);
        cache.slots = 6;
        Tabs a = get(cache, {K(1), K(2), K(3), K(4)}, 1, true, st);
        a.resize(1);                                     // the caller keeps K(1)
        get(cache, {K(5), K(6), K(7), K(8)}, 1, true, st);      // six slots: K(1) and K(2) leave one by one
        CHECK(cache.n.slab_bytes.load() == 2 * SLAB4);
        cache.slots = 100;
        cache.bytes_max = 2 * SLAB4 + 2 * (TAB + AUX) - 1;     // two more keys do not fit
        get(cache, {K(9), K(10)}, 1, true, st);
        // K(3) and K(4) are in the cache and nobody holds them -- but their slab stays alive through K(1), so evicting them frees nothing:
        // the slab of K(5)..K(8) is the idle one.  What is live afterwards: the held slab and the new one.
        CHECK(cache.n.slab_bytes.load() == SLAB4 + 2 * (TAB + AUX) && cache.n.slab_bytes.load() <= cache.bytes_max && blocks() == base + 2);
        CHECK(cached(cache, K(3)) && cached(cache, K(4)) && cached(cache, K(9)) && cached(cache, K(10)));
        CHECK(intact(cache, a[0], K(1)));
        const unsigned long long n0 = cache.n.builds.load();
        cache.bytes_max = 100 * SLAB4;
        CHECK(!cached(cache, K(5)) && !cached(cache, K(8)) && cache.n.builds.load() == n0 + 2);
    }
    CHECK(blocks() == base);
}

// ---- the device refuses: everything nobody holds goes, one retry; refused again: no tables, no error ------------------------
static void out_of_memory(hipStream_t st)
{
    const long base = blocks();
    mockhip::Global &G = mockhip::g();
    {
        KeyTabCache cache;
        small(cache);
        cache.slots = 100;
        get(cache, {K(1), K(2)}, 1, true, st);
        Tabs held = get(cache, {K(3)}, 1, true, st);
        CHECK(blocks() == base + 2);
        G.malloc_fail_in.store(1);
        Tabs n = get(cache, {K(4)}, 1, true, st);
        CHECK(n[0] && intact(cache, n[0], K(4)) && blocks() == base + 2 && cache.n.slab_bytes.load() == 2 * (TAB + AUX));     // K(1), K(2) went
        unsigned long long n0 = cache.n.builds.load();
        CHECK(cached(cache, K(3)) && cached(cache, K(4)) && cache.n.builds.load() == n0 && intact(cache, held[0], K(3)));
        CHECK(!cached(cache, K(1)) && cache.n.builds.load() == n0 + 1);
        // the retry is refused as well: the call succeeds, its keys have no table
        n.clear();
        n0 = cache.n.builds.load();
        G.malloc_fail_len.store(2);
        G.malloc_fail_in.store(1);
        Tabs none = get(cache, {K(20), K(21), K(22), K(23), K(24)}, 1, true, st);
        for (const auto &t : none) CHECK(!t);
        CHECK(cache.n.builds.load() == n0 && blocks() == base + 1 && cached(cache, K(3)) && !cached(cache, K(4)));       // (what nobody held went all the same)
        // ... the first slab of a call built, the second refused twice: the remaining keys have none
        n0 = cache.n.builds.load();
        G.malloc_fail_in.store(2);
        Tabs some = get(cache, {K(30), K(31), K(32), K(33), K(34)}, 1, true, st);
        G.malloc_fail_len.store(1);
        for (unsigned i = 0; i < 4; ++i) CHECK(some[i] && intact(cache, some[i], K(30 + i)));
        CHECK(!some[4] && cache.n.builds.load() == n0 + 4 && intact(cache, held[0], K(3)));
    }
    CHECK(blocks() == base);
}

// ---- pinned tables are never freed: not by the slot bound, the byte bound or the out-of-memory sweep -------------------------
static void pinned(hipStream_t st)
{
    const long base = blocks();
    {
        KeyTabCache cache;
        small(cache);
        Tabs p = get(cache, {K(1), K(2)}, 5000, true, st);
        cache.pin(p);
        cache.pin(p);                                    // (once is enough, twice is harmless)
        const KeyTab *raw1 = p[0].get(), *raw2 = p[1].get();
        const void *t1 = raw1->tab, *t2 = raw2->tab, *w1 = raw1->tab16;
        CHECK(w1 && raw2->tab16);
        p.clear();
        for (unsigned i = 0; i < 12; i += 4) get(cache, {K(10 + i), K(11 + i), K(12 + i), K(13 + i)}, 1, true, st);    // slots, then bytes
        mockhip::g().malloc_fail_in.store(1);
        get(cache, {K(40)}, 1, true, st);
        for (size_t b = 0; b < TAB; ++b) CHECK(((const uint8_t *)t1)[b] == tab_at(K(1).data(), b) && ((const uint8_t *)t2)[b] == tab_at(K(2).data(), b));
        for (size_t b = 0; b < TAB16; ++b) CHECK(((const uint8_t *)w1)[b] == tab16_at(K(1).data(), b));
        CHECK(cache.n.tab16_live.load() == 2);
        // everything unpinned out: the pinned slab and its two 16-bit tables are what is left on the device
        mockhip::g().malloc_fail_len.store(2);
        mockhip::g().malloc_fail_in.store(1);
        get(cache, {K(50)}, 1, true, st);
        mockhip::g().malloc_fail_len.store(1);
        CHECK(blocks() == base + 3 && cache.n.slab_bytes.load() == 2 * (TAB + AUX) && cache.n.tab16_live.load() == 2);
    }
    CHECK(blocks() == base);
}

// ---- no hipFree under the cache's lock ---------------------------------------------------------------------------------------
// The device is held busy by a task that waits on a latch, so a hipFree hangs in its device-wide wait.  While thread A's call sits
// in such a free, a pure-hit call from thread B has to come back: it would not if A still held the lock.
static void wait_for_frees(long n)
{
    for (int i = 0; mockhip::g().frees_started.load() < n; ++i) {
        CHECK(i < 20000);                                // 20 s
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
}
static void hit_returns(KeyTabCache &cache, const Key &k, hipStream_t st, mockhip::Latch &l, const char *when)
{
    std::future<bool> f = std::async(std::launch::async, [&] { Tabs t = get(cache, {k}, 1, false, st); return t[0] && intact(cache, t[0], k); });
    if (f.wait_for(std::chrono::seconds(20)) != std::future_status::ready) {
        fprintf(stderr, "FAILED: a pure-hit call did not return while another call's hipFree waited for the device (%s): hipFree under the cache lock\n", when);
        fflush(stderr);
        l.open();
        _Exit(1);
    }
    CHECK(f.get());
}
static void no_free_under_the_lock(hipStream_t st, hipStream_t sa, hipStream_t sb)
{
    const long base = blocks();
    mockhip::Global &G = mockhip::g();
    {   // an entry that leaves through the slot bound
        KeyTabCache cache;
        small(cache);
        cache.slots = 2;
        get(cache, {K(1)}, 1, true, st);                 // nobody holds K(1): it is the one that will leave, and be freed
        Tabs held = get(cache, {K(2)}, 1, true, st);
        mockhip::Latch l;
        mockhipBlock(g_blocked, &l);
        const long f0 = G.frees_started.load();
        std::thread a([&] { Tabs t = get(cache, {K(3)}, 1, true, sa); CHECK(t[0] && intact(cache, t[0], K(3))); });
        wait_for_frees(f0 + 1);
        hit_returns(cache, K(2), sb, l, "slot bound");
        l.open();
        a.join();
    }
    CHECK(blocks() == base);
    {   // entries that leave through the out-of-memory sweep, then an entry that an insertion replaces
        KeyTabCache cache;
        small(cache);
        cache.slots = 100;
        get(cache, {K(1)}, 1, true, st);
        Tabs held = get(cache, {K(2)}, 1, true, st);
        mockhip::Latch l1, l2;
        mockhipBlock(g_blocked, &l1);
        const long f0 = G.frees_started.load();
        G.malloc_fail_in.store(1);
        std::thread a([&] { Tabs t = get(cache, {K(3)}, 1, true, sa); CHECK(t[0] && intact(cache, t[0], K(3))); });
        wait_for_frees(f0 + 1);                          // A swept K(1) out and waits for the device, the lock dropped
        hit_returns(cache, K(2), sb, l1, "out-of-memory sweep");
        // meanwhile this thread caches the key A is about to build, and lets go of it: A's insertion will replace that entry
        const unsigned long long n0 = cache.n.builds.load();
        get(cache, {K(3)}, 1, true, st);
        CHECK(cache.n.builds.load() == n0 + 1);
        g_block_next_build.store(&l2);                   // A's build makes the device busy again before it inserts
        l1.open();
        wait_for_frees(f0 + 2);                          // the replaced entry's slab
        hit_returns(cache, K(2), sb, l2, "replaced entry");
        l2.open();
        a.join();
        CHECK(cache.n.builds.load() == n0 + 2 && cached(cache, K(3)));
    }
    CHECK(blocks() == base);
}

// ---- eight threads on a tiny cache ---------------------------------------------------------------------------------------------
static void threads()
{
    const long base = blocks();
    {
        KeyTabCache cache;
        small(cache);
        cache.tab16_log2 = 6;                            // (busy after 64 signatures)
        std::mutex mu;
        Tabs pinned_tabs;
        std::vector<Key> pinned_keys;
        std::atomic<int> bad{0};
        std::vector<std::thread> th;
        for (unsigned t = 0; t < 8; ++t)
            th.emplace_back([&, t] {
                hipStream_t st = nullptr;
                CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
                uint32_t r = 12345 + 999 * t;
                const auto rnd = [&r](unsigned m) { r = r * 1664525u + 1013904223u; return (r >> 16) % m; };
                for (int it = 0; it < 60; ++it) {
                    std::vector<Key> ks;
                    for (unsigned i = 0, nk = 1 + rnd(9); i < nk; ++i) { const unsigned tag = rnd(14); ks.push_back(tag < 12 ? K(100 + tag) : off_curve(tag)); }
                    if (it % 7 == 3) mockhip::g().malloc_fail_in.store(1 + rnd(2));
                    if (it % 20 == 11) { mockhip::g().malloc_fail_len.store(2); mockhip::g().malloc_fail_in.store(1); }
                    Tabs out = get(cache, ks, 10, true, st);
                    if (it % 20 == 11) mockhip::g().malloc_fail_len.store(1);
                    for (size_t k = 0; k < ks.size(); ++k) {
                        if (ks[k][0] == OFF_CURVE ? out[k] != nullptr : out[k] && !intact(cache, out[k], ks[k])) bad++;
                        for (size_t j = 0; j < k; ++j) if (ks[j] == ks[k] && out[j] != out[k]) bad++;
                    }
                    if (cache.n.slab_bytes.load() > 1000 * SLAB4 || cache.n.tab16_live.load() < 0 || cache.n.tab16_live.load() > cache.tab16_max) bad++;
                    if (t < 2 && it == 30)                 // a "capture": two threads pin what they hold
                        for (size_t k = 0; k < ks.size(); ++k)
                            if (out[k]) { cache.pin(Tabs{out[k]}); std::lock_guard<std::mutex> lk(mu); pinned_tabs.push_back(out[k]); pinned_keys.push_back(ks[k]); }
                }
                CHECK(hipStreamDestroy(st) == hipSuccess);
            });
        for (auto &t : th) t.join();
        CHECK(bad.load() == 0);
        mockhip::g().malloc_fail_in.store(0);
        mockhip::g().malloc_fail_more.store(0);
        mockhip::g().malloc_fail_len.store(2);          // everything unpinned out (the sweep of a call that ends without a table)
        mockhip::g().malloc_fail_in.store(1);
        get(cache, {K(1)}, 1, true, nullptr);
        mockhip::g().malloc_fail_len.store(1);
        std::set<const KeySlab *> slabs;
        size_t bytes = 0;
        int n16 = 0;
        std::set<const KeyTab *> seen;
        for (size_t i = 0; i < pinned_tabs.size(); ++i) {
            CHECK(intact(cache, pinned_tabs[i], pinned_keys[i]));
            if (!seen.insert(pinned_tabs[i].get()).second) continue;
            if (slabs.insert(pinned_tabs[i]->slab.get()).second) bytes += pinned_tabs[i]->slab->bytes;
            n16 += has16(cache, pinned_tabs[i]) ? 1 : 0;
        }
        CHECK(blocks() == base + (long)slabs.size() + n16);
        CHECK(cache.n.slab_bytes.load() == bytes && cache.n.tab16_live.load() == n16);
        pinned_tabs.clear();
    }
    CHECK(blocks() == base);
}

// ---- device_table_once: made once; a refused allocation leaves the slot empty -------------------------------------------------
static void table_once(hipStream_t st)
{
    const long base = blocks();
    uint8_t *slot = nullptr;
    int queued = 0;
    const auto fill = [&](uint8_t *t) { ++queued; mockhipLaunch(st, [t] { memset(t, 0x77, 32); }); };
    mockhip::g().malloc_fail_in.store(1);
    CHECK(device_table_once(&slot, 32, st, fill) == ERR_OUTOFMEMORY && !slot && queued == 0);
    CHECK(device_table_once(&slot, 32, st, fill) == ERR_OK && slot && queued == 1 && slot[0] == 0x77 && slot[31] == 0x77);
    uint8_t *was = slot;
    CHECK(device_table_once(&slot, 32, st, fill) == ERR_OK && slot == was && queued == 1 && blocks() == base + 1);
    hipFree(slot);
}

int main()
{
    hipStream_t st = nullptr, sa = nullptr, sb = nullptr, cap = nullptr;
    CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithFlags(&sa, hipStreamNonBlocking) == hipSuccess);
    CHECK(hipStreamCreateWithFlags(&sb, hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithFlags(&cap, hipStreamNonBlocking) == hipSuccess);
    CHECK(hipStreamCreateWithFlags(&g_blocked, hipStreamNonBlocking) == hipSuccess);
    mockhip::null_stream();
    table_once(st);
    hit(st, cap);
    miss_under_capture(st, cap);
    miss(st);
    slot_bound(st);
    drop_all(st);
    byte_bound(st);
    slab_with_a_holder_outside(st);
    out_of_memory(st);
    pinned(st);
    no_free_under_the_lock(st, sa, sb);
    threads();
    CHECK(hipDeviceSynchronize() == hipSuccess);
    for (hipStream_t s : {st, sa, sb, cap, g_blocked}) CHECK(hipStreamDestroy(s) == hipSuccess);
    puts("keytab mock ok");
    return 0;
}
