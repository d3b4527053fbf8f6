// bign_keytab.hpp -- one-signer verification: the cache of per-key comb tables, and the make-once helper of G's tables.
// Plain host C++17: no kernel, no curve constant, no template over the curve.  bign_kernels.hip supplies the curve's steps as a
// KeyCurve; tests/hostshim/keytab_mock_main.cpp supplies stand-ins and runs the cache against tests/hostshim/mockhip under
// ASan / UBSan / TSan (tests/test_host_keytab.py).
//
// The comb table of a public key lives in device memory, keyed by (device, curve, key octets); the last `slots` keys per process
// are kept (a table is 278 KiB .. 1 MiB: the card holds as many as anybody wants, the limit only bounds the scan).  A launcher
// holds a reference while it queues its kernels; the table is freed when the last reference goes, and hipFree waits for the device,
// so a kernel already queued never loses its table.
// A slab holds at most `slab_keys` tables, so ONE busy key pins at most that many (4.4 - 16 MiB), and the cache is bounded in BYTES
// as well (`bytes_max` of live slabs): before a new slab is allocated idle slabs go until there is room, and when hipMalloc still
// refuses, every entry nobody holds goes and the allocation is tried once more.  Keys that end up without a table are verified by
// the paths that need none (one signer: the general pipeline; several: the complete-formula kernel) -- slower, same verdicts, no error.
// A key under which 2^tab16_log2 signatures have been verified gets the 16-bit table as well (0.3 / 1 / 2 ms to build -- the work of
// ~2^17 signatures -- against a quarter of the additions saved from then on); at most `tab16_max` keys hold one at a time
// (<= 3 / 7 / 12 GiB per process): a key that becomes busy while they are all taken stays on its 8-bit table.
// The cache has a lock of its own: building a key's tables (host arithmetic, a kernel, a synchronise: 0.2-2 ms) holds it, and
// general verification -- which takes the lock of G's tables -- does not wait behind that.  The two are never nested.
// hipFree is a device-wide wait, so NONE runs under the cache's lock: whatever leaves the cache, is replaced in it or was allocated
// for a build that failed is parked in the call's `dropped` and released after the lock.
#pragma once
#include <algorithm>
#include <atomic>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>
#include "common.hpp"

namespace bee2hip {

// *slot = a device table that is made once: allocate, queue its kernel, wait.  A launch or a wait that fails frees the block again
// (parks it, for a caller that holds a lock hipFree must not run under) and reports `what`, or the failing step when null.
template <class T, class Queue>
static err_t device_table_once(T **slot, size_t bytes, hipStream_t st, Queue &&queue, const char *what = nullptr,
                               std::vector<std::shared_ptr<void>> *park = nullptr)
{
    if (*slot) return ERR_OK;
    void *t = nullptr;
    if (hipMalloc(&t, bytes) != hipSuccess) { (void)hipGetLastError(); return ERR_OUTOFMEMORY; }
    queue(static_cast<T *>(t));
    const char *step = "hipGetLastError()";
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) { step = "hipStreamSynchronize(st)"; e = hipStreamSynchronize(st); }
    if (e == hipSuccess) { *slot = static_cast<T *>(t); return ERR_OK; }
    if (park) park->emplace_back(t, [](void *p) { (void)hipFree(p); });
    else (void)hipFree(t);
    return hip_fail(e, what ? what : step);
}

struct KeyTabCounters {
    std::atomic<size_t> slab_bytes{0};             // live slabs, in the cache or held by somebody
    std::atomic<int> tab16_live{0};
    std::atomic<unsigned long long> builds{0};     // keys whose 8-bit table was built
};
struct KeySlab {                       // tables of keys one call met for the first time, in one device allocation
    KeyTabCounters *n = nullptr;
    void *p = nullptr;
    size_t bytes = 0;
    ~KeySlab() { if (p) { (void)hipFree(p); n->slab_bytes.fetch_sub(bytes); } }
};
struct KeyTab {
    std::shared_ptr<KeySlab> slab;     // (freed with the last of its tables)
    const void *tab = nullptr;         // (2N + 1) x 256 affine points
    const uint8_t *d_key = nullptr;    // the key itself in device memory
    void *tab16 = nullptr;             // N x 65536 affine points (32 / 72 / 128 MiB): once `used` says the key is a busy one
    uint64_t stamp = 0, used = 0;      // signatures verified under the key so far
    ~KeyTab() { if (tab16) { (void)hipFree(tab16); slab->n->tab16_live.fetch_sub(1); } }
};

// what the cache needs to know of a curve, filled in per call
struct KeyCurve {
    std::string id_prefix;                     // (device, curve): in front of the key's octets it names the cache entry
    size_t key_len = 0;
    size_t tab_bytes = 0, aux_bytes = 0;       // a key's 8-bit table; its aux block = the key + the table kernel's starting points
    size_t tab16_bytes = 0;
    int tab16_log2 = 63;                       // the curve's own promotion line
    // is the key a point of the curve?  then out = the starting points (aux_bytes - key_len octets).  Runs on several host threads.
    std::function<bool(const uint8_t *key, uint8_t *out)> on_curve_and_base;
    std::function<void(hipStream_t st, const uint8_t *d_aux, uint8_t *d_tabs, size_t M)> queue_build;      // M tables from M aux blocks
    std::function<void(hipStream_t st, const void *tab, void *t16)> queue_build16;
};

class KeyTabCache {
public:
    using Tabs = std::vector<std::shared_ptr<KeyTab>>;
    size_t slots = 1024;                       // (0.3 - 1 GiB of 8-bit tables when full; tests: tune 21)
    size_t bytes_max = (size_t)8 << 30;
    size_t slab_keys = 16;
    int tab16_max = 96;
    int tab16_log2 = -1;                       // -1: by curve (2^19 on the 256-bit curve, 2^20 on the wider ones); tests / A/B: tune 20
    KeyTabCounters n;                          // (declared before the tables: they count themselves out of it when they go)

    // The tables of nkeys keys (host memory): out[k] = the cached entry, or null for a key that is not a point of the curve (or
    // that the device had no room for).  The keys this process has not met (or has dropped) are built TOGETHER: their starting
    // points on host threads (~35 us a key), one allocation [tables | key, starting points per key], one upload, one launch of
    // the table kernel (0.17 ms for one key, ~0.3 ms for 64: lone wavefronts fill the chip), one synchronisation per slab.
    // credit = signatures of this call under each key (counted towards the 16-bit table of a key when want16).
    err_t tables(const KeyCurve &c, Tabs &out, const uint8_t *keys, size_t nkeys, uint64_t credit, bool want16, hipStream_t st)
    {
        // On a stream that is being captured only queued work is legal.  The 16-bit table of a busy key costs an allocation, a launch
        // and a synchronisation, so a captured call never promotes a key -- it runs on the tables the key has -- and does not count
        // towards the promotion either (a capture queues nothing: the replays verify, and the library does not see them).  The next
        // eager call under the key promotes it as usual.
        const bool capturing = stream_is_capturing(st);
        const int lg = tab16_log2 >= 0 ? tab16_log2 : c.tab16_log2;
        Call x{c, out, keys, credit, lg >= 63 ? ~(uint64_t)0 : (uint64_t)1 << lg, want16 && !capturing, capturing, st};
        out.assign(nkeys, nullptr);
        std::unique_lock<std::mutex> lk(mu_);              // (x is older than lk: what it parks is released after the lock)
        err_t code = look_up(x, nkeys);
        if (code != ERR_OK || x.miss.empty()) return code;
        // a key this process has not met needs an allocation, an upload and a synchronisation: none of that is legal on a stream
        // that is being captured (and would kill the capture).  Say so instead: verify once under the key outside the capture.
        if (capturing)
            return hip_fail(hipErrorStreamCaptureUnsupported, "key-table miss under stream capture: verify once under each key before capturing");
        code = host_bases(x);
        for (size_t g0 = 0; code == ERR_OK && g0 < x.good.size(); g0 += slab_keys) {
            const size_t M = std::min(slab_keys, x.good.size() - g0);
            if (!make_room(x, lk, M * (c.tab_bytes + c.aux_bytes))) break;     // the remaining keys stay without a table: the callers' table-free paths
            code = build_slab(x, g0, M);
            if (code == ERR_OK) code = insert(x, g0, M);
        }
        if (code != ERR_OK) return code;
        for (size_t k = 0; k < nkeys; ++k) if (x.dup_of[k] != (size_t)-1) out[k] = out[x.dup_of[k]];
        return ERR_OK;
    }

    // A stream CAPTURE bakes the tables' addresses into the graph, and nothing tells the library when that graph dies: the tables
    // a capture refers to are pinned for the life of the cache (a reference that is never dropped), so neither the LRU nor a
    // later call's eviction can free memory a replay will read.  Bounded by the distinct keys ever captured.
    void pin(const Tabs &kts)
    {
        std::lock_guard<std::mutex> lk(mu_);
        for (const auto &t : kts)
            if (t && std::find(pinned_.begin(), pinned_.end(), t) == pinned_.end()) pinned_.push_back(t);
    }

    // the tables' addresses as they are now (another thread may be giving a key its 16-bit table); null for a key without an entry
    void view(const Tabs &kts, const void **tab, const void **tab16)
    {
        std::lock_guard<std::mutex> lk(mu_);
        for (size_t k = 0; k < kts.size(); ++k) {
            tab[k] = kts[k] ? kts[k]->tab : nullptr;
            tab16[k] = kts[k] ? kts[k]->tab16 : nullptr;
        }
    }

    // Every entry leaves the cache (tests: a known starting state, room among the tab16_max).  As with an eviction, a table somebody
    // still holds -- a launcher, a captured graph -- lives on until they let go; hipFree runs after the lock.
    void drop_all()
    {
        Tabs gone;
        std::lock_guard<std::mutex> lk(mu_);               // (gone is older than lk)
        gone.reserve(map_.size());
        for (auto &e : map_) gone.push_back(std::move(e.second));
        map_.clear();
    }

private:
    struct Call {                                          // one call of tables()
        const KeyCurve &c;
        Tabs &out;
        const uint8_t *keys;
        uint64_t credit, after;                            // `after` signatures a key is a busy one
        bool want16, capturing;
        hipStream_t st;
        std::vector<size_t> miss, dup_of;                  // first occurrence of every key the cache does not hold; of a later one, the first
        std::vector<size_t> good;                          // the missing keys that are points of the curve (positions in miss)
        std::vector<uint8_t> bases;                        // ... and their starting points
        std::shared_ptr<KeySlab> slab;                     // the slab that is being built
        size_t pending_free = 0;                           // slab bytes that return when `dropped` is released
        std::vector<std::shared_ptr<void>> dropped;        // what hipFree is owed for: released without the lock
        const uint8_t *key(size_t k) const { return keys + c.key_len * k; }
        std::string id(size_t k) const { return c.id_prefix + std::string(reinterpret_cast<const char *>(key(k)), c.key_len); }
    };

    std::mutex mu_;
    std::unordered_map<std::string, std::shared_ptr<KeyTab>> map_;
    Tabs pinned_;
    uint64_t clock_ = 0;

    // made from the 8-bit table like G's.  No room, on the device or among the tab16_max: not an error, the 8-bit table serves
    err_t promote(Call &x, KeyTab &t)
    {
        if (!x.want16 || t.tab16 || t.used < x.after || n.tab16_live.load() >= tab16_max) return ERR_OK;
        const err_t code = device_table_once(&t.tab16, x.c.tab16_bytes, x.st, [&](void *t16) { x.c.queue_build16(x.st, t.tab, t16); },
                                             "bign_gtable16_kernel (key)", &x.dropped);
        if (t.tab16) n.tab16_live.fetch_add(1);
        return code == ERR_OUTOFMEMORY ? ERR_OK : code;
    }

    err_t look_up(Call &x, size_t nkeys)
    {
        std::unordered_map<std::string, size_t> miss_at;   // id -> position in miss
        x.dup_of.assign(nkeys, (size_t)-1);
        for (size_t k = 0; k < nkeys; ++k) {
            std::string id = x.id(k);
            const auto it = map_.find(id);
            if (it != map_.end()) {
                KeyTab &t = *it->second;
                t.stamp = ++clock_;
                if (!x.capturing) t.used += x.credit;
                const err_t code = promote(x, t);
                if (code != ERR_OK) return code;
                x.out[k] = it->second;
                continue;
            }
            const auto m = miss_at.find(id);
            if (m != miss_at.end()) { x.dup_of[k] = x.miss[m->second]; continue; }
            miss_at.emplace(std::move(id), x.miss.size());
            x.miss.push_back(k);
        }
        return ERR_OK;
    }

    // on the curve?  then the starting points -- host threads when there are many keys
    err_t host_bases(Call &x)
    {
        const size_t nm = x.miss.size(), B = x.c.aux_bytes - x.c.key_len;
        x.bases.resize(nm * B);
        std::vector<char> on_curve(nm, 0);
        std::atomic<int> threw{0};                         // (an exception must not leave a worker thread: bad_alloc in a resize)
        const auto work = [&](size_t from, size_t to) {
            try {
                for (size_t i = from; i < to; ++i) on_curve[i] = x.c.on_curve_and_base(x.key(x.miss[i]), x.bases.data() + i * B) ? 1 : 0;
            } catch (...) { threw.store(1); }
        };
        const size_t nthr = std::min<size_t>(16, nm / 4);
        if (nthr >= 2) {
            std::vector<std::thread> th;
            const size_t per = (nm + nthr - 1) / nthr;
            size_t started = 0;
            try {
                for (; started < nthr; ++started) th.emplace_back(work, std::min(nm, started * per), std::min(nm, (started + 1) * per));
            } catch (...) {                                // no more threads to be had: the rest on this one
                work(std::min(nm, started * per), nm);
            }
            for (auto &t : th) t.join();
        } else work(0, nm);
        if (threw.load()) return ERR_OUTOFMEMORY;
        for (size_t i = 0; i < nm; ++i) if (on_curve[i]) x.good.push_back(i);
        return ERR_OK;
    }

    void evict_lru(Call &x)                                // the entry with the oldest stamp leaves the cache (freed when its last user lets go)
    {
        if (map_.empty()) return;
        auto old = map_.begin();
        for (auto it = map_.begin(); it != map_.end(); ++it) if (it->second->stamp < old->second->stamp) old = it;
        x.dropped.push_back(std::move(old->second));
        map_.erase(old);
    }

    // The BYTE bound evicts by slab: a slab's memory returns only when ALL of its tables are gone and nobody holds one, so the unit
    // that leaves is the idle slab whose most recent use is the oldest.  Idle = every live table of the slab is in the cache and
    // held by the cache alone; a slab with a table that left earlier and is still held (by a launcher, a captured graph) would not
    // give its bytes back.  Returns the bytes that will be freed once `dropped` is released, 0 when no idle slab is left.
    size_t evict_idle_slab(Call &x)
    {
        struct Seen { uint64_t newest = 0; long tabs = 0, refs = 0; bool held = false; };
        std::unordered_map<const KeySlab *, Seen> slabs;
        for (const auto &kv : map_) {
            Seen &e = slabs[kv.second->slab.get()];
            e.newest = std::max(e.newest, kv.second->stamp);
            e.tabs += 1;
            e.refs = kv.second->slab.use_count();
            e.held |= kv.second.use_count() != 1;
        }
        const KeySlab *victim = nullptr;
        uint64_t oldest = ~(uint64_t)0;
        for (const auto &kv : slabs)
            if (!kv.second.held && kv.second.refs == kv.second.tabs && kv.second.newest < oldest) { oldest = kv.second.newest; victim = kv.first; }
        if (!victim) return 0;
        const size_t bytes = victim->bytes;
        for (auto it = map_.begin(); it != map_.end();)
            if (it->second->slab.get() == victim) { x.dropped.push_back(std::move(it->second)); it = map_.erase(it); } else ++it;
        return bytes;
    }

    // x.slab = `need` bytes of device memory, within the byte bound as far as idle slabs allow.  When the device refuses, everything
    // nobody is using goes -- released HERE, with lk dropped, because the retry needs the memory back now -- then one more try.
    // (Another thread may cache one of this call's keys meanwhile: insert() then replaces its entry.)  false: no memory.
    bool make_room(Call &x, std::unique_lock<std::mutex> &lk, size_t need)
    {
        for (size_t live; (live = n.slab_bytes.load()) - std::min(x.pending_free, live) + need > bytes_max;) {
            const size_t freed = evict_idle_slab(x);
            if (!freed) break;                             // (it never empties the cache without freeing a byte)
            x.pending_free += freed;
        }
        x.slab = std::make_shared<KeySlab>();
        x.slab->n = &n;
        if (hipMalloc(&x.slab->p, need) != hipSuccess) {
            (void)hipGetLastError();
            x.slab->p = nullptr;
            for (auto it = map_.begin(); it != map_.end();)
                if (it->second.use_count() == 1) { x.dropped.push_back(std::move(it->second)); it = map_.erase(it); } else ++it;
            lk.unlock();
            x.dropped.clear();
            x.pending_free = 0;
            lk.lock();
            if (hipMalloc(&x.slab->p, need) != hipSuccess) {
                (void)hipGetLastError();
                x.slab->p = nullptr;
                return false;
            }
        }
        x.slab->bytes = need;
        n.slab_bytes.fetch_add(need);
        return true;
    }

    err_t build_slab(Call &x, size_t g0, size_t M)
    {
        const KeyCurve &c = x.c;
        const hipStream_t st = x.st;
        uint8_t *d_tabs = reinterpret_cast<uint8_t *>(x.slab->p), *d_aux = d_tabs + M * c.tab_bytes;
        std::vector<uint8_t> aux(M * c.aux_bytes);
        for (size_t j = 0; j < M; ++j) {
            const size_t i = x.good[g0 + j];
            memcpy(aux.data() + j * c.aux_bytes, x.key(x.miss[i]), c.key_len);
            memcpy(aux.data() + j * c.aux_bytes + c.key_len, x.bases.data() + i * (c.aux_bytes - c.key_len), c.aux_bytes - c.key_len);
        }
        B2H_TRY(hipMemcpyAsync(d_aux, aux.data(), aux.size(), hipMemcpyHostToDevice, st));
        c.queue_build(st, d_aux, d_tabs, M);
        B2H_TRY(hipGetLastError());
        B2H_TRY(hipStreamSynchronize(st));                 // (aux goes out of scope; other streams may use the tables next)
        return ERR_OK;
    }

    err_t insert(Call &x, size_t g0, size_t M)
    {
        const KeyCurve &c = x.c;
        uint8_t *d_tabs = reinterpret_cast<uint8_t *>(x.slab->p), *d_aux = d_tabs + M * c.tab_bytes;
        for (size_t j = 0; j < M; ++j) {
            const size_t k = x.miss[x.good[g0 + j]];
            auto t = std::make_shared<KeyTab>();
            t->slab = x.slab;
            t->tab = d_tabs + j * c.tab_bytes;
            t->d_key = d_aux + j * c.aux_bytes;
            t->stamp = ++clock_;
            t->used = x.credit;
            n.builds.fetch_add(1);
            const err_t code = promote(x, *t);
            if (code != ERR_OK) return code;
            if (map_.size() >= slots) evict_lru(x);
            std::shared_ptr<KeyTab> &e = map_[x.id(k)];
            if (e) x.dropped.push_back(std::move(e));      // (another thread cached the key while make_room had the lock dropped)
            e = t;
            x.out[k] = t;
        }
        x.slab.reset();
        return ERR_OK;
    }
};

}  // namespace bee2hip
