// TEST INFRASTRUCTURE: the HOST side of libbee2hip.so -- bee2_amd/csrc/staging.hpp (error record, scratch pool, per-thread
// staging, host fallback, the duplex pipeline of large in-place batches) and multi.hip (the persistent worker pool behind the
// *_multi entries) -- compiled with g++ against tests/hostshim/mockhip (streams = threads, device memory = heap) so that it
// runs under -fsanitize=thread and -fsanitize=address,undefined on a box without a GPU.  The kernels are stand-ins (a byte
// transform queued on the stream); what is under test is the library's own synchronisation: every result is compared with
// the same transform applied directly, every failure path must leave the contract of *done_units intact, and the sanitizer
// must stay silent.  Built and run by tests/test_host_sanitizers.py.  Nothing here ships.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <new>
#include "../../bee2_amd/csrc/staging.hpp"

namespace bee2hip {
err_t upload_beltH(const uint8_t *) { return ERR_OK; }
err_t upload_beltH_bign(const uint8_t *) { return ERR_OK; }
}  // namespace bee2hip

// ---- the single-device entries multi.hip dispatches to: CPU stand-ins with the real contracts -------------------------
static inline octet tf(octet x, size_t unit) { return (octet)(x * 5 + 1 + (octet)(unit * 7)); }      // "kernel": depends on the unit's index
static std::atomic<int> g_calls{0};
extern "C" {
err_t bee2hip_set_device(int d) { return hipSetDevice(d) == hipSuccess ? ERR_OK : ERR_BEE2HIP_DEVICE; }
err_t bee2hip_bashF_batch(octet *states, size_t n)
{
    g_calls.fetch_add(1);
    for (size_t i = 0; i < n; ++i) hostp::bashF(states + 192 * i);
    return ERR_OK;
}
struct ctr_st { u32 key[8]; u32 ctr[4]; octet block[16]; size_t reserved; };
err_t bee2hip_beltCTR_bulk(void *buf, size_t count, void *state)
{
    g_calls.fetch_add(1);
    ctr_st *st = (ctr_st *)state;
    hostp::ctr_blocks(hostT(), (octet *)buf, count, st->key, st->ctr, st->block, &st->reserved);
    return ERR_OK;
}
err_t bee2hip_bashF_batch_dev(void *d_states, size_t n, void *stream)
{
    octet *p = (octet *)d_states;
    mockhipLaunch(as_stream(stream), [p, n] { for (size_t i = 0; i < n; ++i) hostp::bashF(p + 192 * i); });
    return n == 12345 ? ERR_BAD_INPUT : ERR_OK;          // (a launcher that queues work and THEN reports an error: drain() must still wait)
}
#define STUB(name, ...) err_t name(__VA_ARGS__) { return ERR_OK; }
STUB(bee2hip_beltCTR_blocks_dev, void *, size_t, const u32 *, const u32 *, uint64_t, void *)
STUB(bee2hip_bignVerify_batch, const bign_params *, const octet *, size_t, const octet *, const octet *, const octet *, size_t, err_t *)
STUB(bee2hip_bignVerify_keyed_batch, const bign_params *, const octet *, size_t, const octet *, const octet *, const octet *, size_t, const u32 *, size_t, err_t *)
STUB(bee2hip_bignVerify_onekey_batch, const bign_params *, const octet *, size_t, const octet *, const octet *, const octet *, size_t, err_t *)
STUB(bee2hip_bignSign2_batch, const bign_params *, const octet *, size_t, const octet *, const octet *, const void *, size_t, size_t, octet *, err_t *)
STUB(bee2hip_bashHash_beltMAC_batch, const octet *, size_t, size_t, size_t, const octet *, size_t, octet *, octet *)
STUB(bee2hip_hash_ragged, size_t, const octet *, const uint64_t *, size_t, octet *)
STUB(bee2hip_bignVerifyL_batch_dev, size_t, const octet *, size_t, const void *, const void *, const void *, size_t, void *, void *)
STUB(bee2hip_bignVerifyL_onekey_batch_dev, size_t, const octet *, size_t, const void *, const void *, const octet *, size_t, void *, void *)
STUB(bee2hip_bignVerifyL_keyed_batch_dev, size_t, const octet *, size_t, const void *, const void *, const octet *, size_t, const void *, size_t, void *, void *)
STUB(bee2hip_bashHash_beltMAC_batch_dev, const void *, size_t, size_t, size_t, const octet *, size_t, void *, void *, void *)
}
#include "../../bee2_amd/csrc/multi.hip"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

// the "kernel" of the duplex tests: transforms units [first, first + cnt) of the device chunk on the stream
static err_t launch_tf(octet *d, size_t unit_bytes, size_t first, size_t cnt, hipStream_t st)
{
    mockhipLaunch(st, [=] { for (size_t u = 0; u < cnt; ++u) for (size_t b = 0; b < unit_bytes; ++b) d[u * unit_bytes + b] = tf(d[u * unit_bytes + b], first + u); });
    return ERR_OK;
}
static void fill(std::vector<octet> &v, unsigned seed) { for (size_t i = 0; i < v.size(); ++i) v[i] = (octet)((i * 2654435761u + seed) >> 13); }

static void duplex_ok(size_t unit_bytes, size_t units, size_t chunk)
{
    std::vector<octet> host(unit_bytes * units), want;
    fill(host, (unsigned)(units + chunk));
    want = host;
    for (size_t u = 0; u < units; ++u) for (size_t b = 0; b < unit_bytes; ++b) want[u * unit_bytes + b] = tf(want[u * unit_bytes + b], u);
    void *dev = nullptr;
    CHECK(hipMalloc(&dev, host.size()) == hipSuccess);
    size_t done = 777;
    const err_t code = duplex_inplace(host.data(), (octet *)dev, unit_bytes, units, chunk,
                                      [=](octet *d, size_t first, size_t cnt, hipStream_t st) { return launch_tf(d, unit_bytes, first, cnt, st); }, &done);
    CHECK(code == ERR_OK && done == units && host == want);
    hipFree(dev);
}

// mode 1: the launcher reports an error at chunk `bad`; 2: it throws std::bad_alloc there; 3: it throws something else
static void duplex_fails(size_t units, size_t chunk, size_t bad, int mode)
{
    const size_t ub = 16;
    std::vector<octet> host(ub * units), orig;
    fill(host, 99);
    orig = host;
    void *dev = nullptr;
    CHECK(hipMalloc(&dev, host.size()) == hipSuccess);
    size_t done = 777, seen = 0;
    const err_t code = duplex_inplace(host.data(), (octet *)dev, ub, units, chunk, [&](octet *d, size_t first, size_t cnt, hipStream_t st) -> err_t {
        if (seen++ == bad) {
            if (mode == 2) throw std::bad_alloc();
            if (mode == 3) throw 42;
            return ERR_BEE2HIP_DEVICE;
        }
        return launch_tf(d, ub, first, cnt, st);
    }, &done);
    CHECK(code == (mode == 2 ? ERR_OUTOFMEMORY : ERR_BEE2HIP_DEVICE));       // a code, never an exception
    CHECK(done <= bad * chunk && done % chunk == 0);
    // the contract: the leading `done` units are transformed in the caller's buffer, everything behind them is untouched
    for (size_t u = 0; u < units; ++u)
        for (size_t b = 0; b < ub; ++b) CHECK(host[u * ub + b] == (u < done ? tf(orig[u * ub + b], u) : orig[u * ub + b]));
    hipFree(dev);
}

static void pool_and_fallback()
{
    // scratch_for_stream from many threads on the NULL stream (keyed by thread) and on private streams; blocks grow; threads exit
    std::vector<std::thread> th;
    std::atomic<int> bad{0};
    for (int t = 0; t < 8; ++t)
        th.emplace_back([t, &bad] {
            hipStream_t st = nullptr;
            if (t & 1) { if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { bad++; return; } }
            for (size_t sz = 64; sz <= 65536; sz *= 4) {
                void *p = nullptr;
                if (scratch_for_stream(st, t & 3, sz, &p) != ERR_OK || !p) { bad++; continue; }
                octet *q = (octet *)p;
                mockhipLaunch(st, [q, sz, t] { memset(q, t, sz); });
                if (hipStreamSynchronize(st) != hipSuccess || q[sz - 1] != (octet)t) bad++;
            }
            if (st) { scratch_release_stream(st); hipStreamDestroy(st); }
        });
    for (auto &t : th) t.join();
    CHECK(bad.load() == 0);
    // with_host: a GPU path that fails twice is finished on the host and counted; ERR_BAD_INPUT is reported, not retried
    g_force.store(FORCE_AUTO);
    int host_runs = 0, gpu_runs = 0;
    const unsigned long long fb0 = g_n_fallback.load();
    CHECK(with_host(K_PARALLEL, 1 << 20, "test", [&]() -> err_t { ++gpu_runs; return ERR_BEE2HIP_DEVICE; }, [&] { ++host_runs; }) == ERR_OK);
    CHECK(gpu_runs == 2 && host_runs == 1 && g_n_fallback.load() == fb0 + 1);
    CHECK(with_host(K_PARALLEL, 1 << 20, "test", [&]() -> err_t { throw std::bad_alloc(); }, [&] { ++host_runs; }) == ERR_OK && host_runs == 2);
    CHECK(with_host(K_PARALLEL, 1 << 20, "test", [&]() -> err_t { return ERR_BAD_INPUT; }, [&] { ++host_runs; }) == ERR_BAD_INPUT && host_runs == 2);
    g_force.store(FORCE_GPU);
    CHECK(with_host(K_PRIM, 16, "test", [&]() -> err_t { return ERR_BEE2HIP_DEVICE; }, [&] { ++host_runs; }) == ERR_BEE2HIP_DEVICE && host_runs == 2);
    g_force.store(FORCE_AUTO);
    // a refused device allocation is ERR_OUTOFMEMORY, and the pool entry stays usable
    void *p = nullptr;
    mockhip::g().malloc_fail_in.store(1);
    CHECK(scratch_for_stream(nullptr, 3, 1 << 22, &p) == ERR_OUTOFMEMORY);
    CHECK(scratch_for_stream(nullptr, 3, 1 << 22, &p) == ERR_OK && p);
}

static void worker_pool()
{
    // the *_multi entries from several host threads at once: one batch over all (logical) devices at a time, results exact
    const size_t n = 301;
    std::vector<std::thread> th;
    std::atomic<int> bad{0};
    for (int t = 0; t < 4; ++t)
        th.emplace_back([t, n, &bad] {
            std::vector<octet> a(192 * n), want;
            fill(a, 1000 + t);
            want = a;
            for (size_t i = 0; i < n; ++i) hostp::bashF(want.data() + 192 * i);
            if (bee2hip_bashF_batch_multi(a.data(), n, 1 + t) != ERR_OK || a != want) bad++;
            // resident shards: worker i launches on its own stream and drains it -- the data must be final when the call returns
            const int nd = 2;
            std::vector<std::vector<octet>> sh(nd, std::vector<octet>(192 * 40)), w2;
            for (int i = 0; i < nd; ++i) fill(sh[i], 7 * t + i);
            w2 = sh;
            for (int i = 0; i < nd; ++i) for (size_t k = 0; k < 40; ++k) hostp::bashF(w2[i].data() + 192 * k);
            void *ptrs[nd] = {sh[0].data(), sh[1].data()};
            size_t cnt[nd] = {40, 40};
            if (bee2hip_bashF_batch_multi_dev(ptrs, cnt, nd) != ERR_OK || sh != w2) bad++;
        });
    for (auto &t : th) t.join();
    CHECK(bad.load() == 0);
    // a launcher that queued work and then reported an error: the call returns the error AND the queued work is finished
    std::vector<octet> s(192 * 12345), w;
    fill(s, 5);
    w = s;
    for (size_t k = 0; k < 12345; ++k) hostp::bashF(w.data() + 192 * k);
    void *ptrs[1] = {s.data()};
    size_t cnt[1] = {12345};
    CHECK(bee2hip_bashF_batch_multi_dev(ptrs, cnt, 1) == ERR_BAD_INPUT);
    CHECK(s == w);                                      // nothing was still in flight when the call came back
    // CTR over several logical devices leaves the state exactly as ONE serial call does
    ctr_st st0;
    for (int i = 0; i < 8; ++i) st0.key[i] = 0x01020304u * (i + 1);
    for (int i = 0; i < 4; ++i) st0.ctr[i] = 0xFFFFFFF0u + i;
    memset(st0.block, 0, 16); st0.reserved = 0;
    std::vector<octet> m(16 * 1000 + 5), m1;
    fill(m, 3);
    m1 = m;
    ctr_st a = st0, b = st0;
    CHECK(bee2hip_beltCTR_bulk(m1.data(), m1.size(), &a) == ERR_OK);
    CHECK(bee2hip_beltCTR_bulk_multi(m.data(), m.size(), &b, 3) == ERR_OK);
    CHECK(m == m1 && !memcmp(&a, &b, sizeof a));
}

// ---- Stage: layout, pinned / device choice, the round trip through both, zero-length copies, secrets on every way out ----
// a staged call as the entries write them: two inputs and an output, the first input secret; `how` picks the way out
// (0 return at the end, 1 early error return, 2 std::bad_alloc); *where = the staging block, for the caller to inspect afterwards
static err_t staged_call(size_t na, size_t nb, const octet *a, const octet *b, octet *out, int how, octet **where, size_t *o_sec)
{
    Stage sg(1, false, "stage_helper");
    const size_t o_a = sg.add(na), o_b = sg.add(nb), o_out = sg.add(na + nb);
    sg.secret(o_a, na);
    B2H_OK(sg.open(16));
    *where = sg.at(0);
    *o_sec = o_a;
    B2H_OK(sg.in(o_a, a, na));
    B2H_OK(sg.in(o_b, b, nb));
    if (how == 1) return ERR_BAD_INPUT;
    if (how == 2) throw std::bad_alloc();
    octet *pa = sg.at(o_a), *pb = sg.at(o_b), *po = sg.at(o_out);
    mockhipLaunch(nullptr, [=] { for (size_t i = 0; i < na; ++i) po[i] = tf(pa[i], i); for (size_t i = 0; i < nb; ++i) po[na + i] = tf(pb[i], na + i); });
    return sg.out(out, o_out, na + nb);
}
static void stage_helper()
{
    // offsets: 16-aligned, in the order added, no overlap, and what the chained (x + 15) & ~15 of the entries gave
    const size_t orders[][6] = {{0, 1, 15, 16, 17, 4097}, {4097, 17, 16, 15, 1, 0}, {16, 0, 4097, 1, 17, 15}, {15, 4097, 0, 17, 16, 1},
                                {1, 1, 16, 16, 0, 0}};
    for (const auto &order : orders) {
        Stage sg(0, false, "stage_helper");
        size_t hand = 0, end = 0;
        for (const size_t n : order) {
            const size_t off = sg.add(n);
            hand = (hand + 15) & ~(size_t)15;
            CHECK(off == hand && off % 16 == 0 && off >= end && up16(off) == off);
            hand += n;
            end = off + n;
        }
        g_pinned_limit = end + 8;                              // the byte count open() asks for is the hand formula's total + the slack
        CHECK(sg.open(8) == ERR_OK && in_pinned(sg.at(0)));
        g_pinned_limit = end + 7;
        CHECK(sg.open(8) == ERR_OK && !in_pinned(sg.at(0)));
        g_pinned_limit = PINNED_MAX;
    }
    // pinned or device: the byte count given to need() decides, to the byte
    const auto where = [](size_t total, size_t slack, bool chain) {
        Stage sg(2, chain, "stage_helper");
        sg.add(total - slack);
        CHECK(sg.open(slack) == ERR_OK);
        return in_pinned(sg.at(0));
    };
    CHECK(where(PINNED_MAX, 0, false) && !where(PINNED_MAX + 1, 0, false));
    CHECK(where(PINNED_MAX, 16, false) && !where(PINNED_MAX + 1, 16, false));
    CHECK(where(2048, 0, true) && !where(2049, 0, true) && where(2048, 16, true) && !where(2049, 16, true));
    g_pinned_limit = 0;
    CHECK(!where(1, 0, false) && !where(16, 16, true) && !where(PINNED_MAX, 0, false));
    g_pinned_limit = PINNED_MAX;
    // round trip, secrets and exits in both modes
    for (int device = 0; device < 2; ++device) {
        g_pinned_limit = device ? 0 : PINNED_MAX;
        const size_t shapes[][2] = {{1, 0}, {15, 17}, {16, 16}, {17, 4097}, {0, 33}};
        for (const auto &sh : shapes) {
            const size_t na = sh[0], nb = sh[1];
            std::vector<octet> a(na), b(nb), out(na + nb, 0xEE), want(na + nb);
            fill(a, 11); fill(b, 12);
            for (size_t i = 0; i < na; ++i) a[i] |= 1;         // (no zero octet in the secret: a wipe shows)
            for (size_t i = 0; i < na + nb; ++i) want[i] = tf(i < na ? a[i] : b[i - na], i);
            for (int how = 0; how < 3; ++how) {
                octet *blk = nullptr;
                size_t o_sec = 0;
                std::fill(out.begin(), out.end(), 0xEE);
                err_t code = ERR_OK;
                try { code = staged_call(na, nb, a.data(), b.data(), out.data(), how, &blk, &o_sec); }
                catch (const std::bad_alloc &) { CHECK(how == 2); code = ERR_OUTOFMEMORY; }
                CHECK(code == (how == 0 ? ERR_OK : how == 1 ? ERR_BAD_INPUT : ERR_OUTOFMEMORY));
                CHECK(in_pinned(blk) == !device);
                if (how == 0) CHECK(out == want);
                else for (octet x : out) CHECK(x == 0xEE);
                // the staging block afterwards: the secret part reads zero, the part behind it is what was staged
                std::vector<octet> img(up16(na) + nb);
                CHECK(hipMemcpy(img.data(), blk, img.size(), hipMemcpyDeviceToHost) == hipSuccess);
                for (size_t i = 0; i < na; ++i) CHECK(img[o_sec + i] == 0);
                for (size_t i = 0; i < nb; ++i) CHECK(img[up16(na) + i] == b[i]);
            }
        }
    }
    {   // zero-length in / out touch nothing, null host pointers included
        Stage sg(1, false, "stage_helper");
        const size_t o = sg.add(32);
        CHECK(sg.open() == ERR_OK);
        memset(sg.at(o), 0x5A, 32);
        CHECK(sg.in(o, nullptr, 0) == ERR_OK && sg.out(nullptr, o, 0) == ERR_OK);
        for (size_t i = 0; i < 32; ++i) CHECK(sg.at(o)[i] == 0x5A);
    }
    {   // open() refused: ERR_OUTOFMEMORY, and the Stage that marked a secret goes without dereferencing anything
        g_pinned_limit = 0;
        octet *blk = nullptr;
        size_t o_sec = 0;
        octet a[16] = {1}, b[1] = {2}, out[17];
        mockhip::g().malloc_fail_in.store(1);
        // (slot 1 holds fewer than 1 MiB: the request has to allocate)
        std::vector<octet> big(1 << 20), big_out(16 + big.size());
        CHECK(staged_call(16, big.size(), a, big.data(), big_out.data(), 0, &blk, &o_sec) == ERR_OUTOFMEMORY && blk == nullptr);
        CHECK(staged_call(16, 1, a, b, out, 0, &blk, &o_sec) == ERR_OK && blk != nullptr);
        g_pinned_limit = PINNED_MAX;
    }
}

// ---- RaggedPart: the ragged part of a Stage, as the ragged host-pointer entries use it ----
// n records cut out of a caller array from octet `first` on; the array carries a guard octet (and `first` octets nobody may
// touch) in front and a guard behind.  lens has n entries.
static void ragged_case(size_t first, const std::vector<size_t> &lens, bool device)
{
    const size_t n = lens.size();
    std::vector<uint64_t> offs(n + 1);
    offs[0] = first;
    for (size_t i = 0; i < n; ++i) offs[i + 1] = offs[i] + lens[i];
    const size_t total = (size_t)(offs[n] - offs[0]);
    // caller's array: 16-aligned base, so that (data + first) mod 16 = first mod 16
    std::vector<octet> raw(first + total + 1 + 16), back;
    octet *data = raw.data() + ((16 - ((uintptr_t)raw.data() & 15)) & 15);
    for (size_t i = 0; i < first + total + 1; ++i) data[i] = (octet)(i * 37 + 11 + n);
    g_pinned_limit = device ? 0 : PINNED_MAX;
    Stage sg(1, false, "ragged_part");
    const size_t o_front = sg.add(5);                           // (something in front: the part starts at a later offset)
    RaggedPart part(sg, offs.data(), n), none(sg, nullptr, n);
    const size_t o_mid = sg.add(3);
    part.add_offs(sg);
    none.add_offs(sg);
    const size_t o_end = sg.add(1);
    CHECK(part.first == first && part.total == total && part.lead == (first & 15));
    CHECK(part.o_data == up16(o_front + 5) && o_mid == up16(part.o_data + part.lead + total));
    CHECK(part.o_off == up16(o_mid + 3) && o_end == up16(part.o_off + (n + 1) * 8));        // the absent part added nothing
    CHECK(none.total == 0 && none.lead == 0);
    CHECK(sg.open(16) == ERR_OK && in_pinned(sg.at(0)) == !device);
    CHECK(none.data(sg) == nullptr && none.offs(sg) == nullptr);
    CHECK(none.in(sg, nullptr) == ERR_OK && none.out(sg, nullptr) == ERR_OK);
    CHECK(part.in(sg, total ? data : nullptr) == ERR_OK);       // no octets: a null array is accepted
    // what was staged (read back through the runtime: the block may be "device" memory)
    std::vector<octet> img(o_end + 1);
    CHECK(hipMemcpy(img.data(), sg.at(0), img.size(), hipMemcpyDeviceToHost) == hipSuccess);
    CHECK(part.data(sg) == sg.at(part.o_data) && part.offs(sg) == sg.at(part.o_off));
    CHECK(((uintptr_t)sg.at(0) & 15) == 0);
    CHECK(((uintptr_t)(part.data(sg) + part.lead) & 15) == ((uintptr_t)(data + first) & 15));
    for (size_t i = 0; i < total; ++i) CHECK(img[part.o_data + part.lead + i] == data[first + i]);
    for (size_t i = 0; i <= n; ++i) {
        uint64_t v;
        memcpy(&v, img.data() + part.o_off + 8 * i, 8);
        CHECK(v == offs[i] - first + part.lead);
    }
    // out(): a "kernel" transforms the staged text in place; exactly [first, first + total) comes back
    octet *txt = part.data(sg) + part.lead;
    mockhipLaunch(nullptr, [=] { for (size_t i = 0; i < total; ++i) txt[i] = tf(txt[i], i); });
    back.assign(1 + first + total + 1, 0xA5);
    CHECK(part.out(sg, total ? back.data() + 1 : nullptr) == ERR_OK);
    for (size_t i = 0; i < back.size(); ++i) {
        const bool mine = i >= 1 + first && i < 1 + first + total;
        CHECK(back[i] == (mine ? tf(data[i - 1], i - 1 - first) : 0xA5));
    }
    g_pinned_limit = PINNED_MAX;
}
static void ragged_part()
{
    for (int device = 0; device < 2; ++device) {
        for (size_t first = 0; first <= 16; ++first) {
            const size_t f = first < 16 ? first : 4099;
            ragged_case(f, {0}, device);
            ragged_case(f, {1}, device);
            ragged_case(f, {33}, device);
            ragged_case(f, {0, 0, 0}, device);
            ragged_case(f, {5, 0, 16}, device);
            ragged_case(f, {0, 31, 1}, device);
        }
    }
    // offsets_rise: a descending pair is refused wherever it is
    const uint64_t up[5] = {7, 7, 9, 20, 20}, d0[5] = {7, 6, 9, 20, 20}, dl[5] = {7, 7, 9, 20, 19}, d1[2] = {1, 0};
    CHECK(offsets_rise(up, 4) && offsets_rise(up, 0) && !offsets_rise(d0, 4) && !offsets_rise(dl, 4) && !offsets_rise(d1, 1));
    CHECK(offsets_rise(dl, 3));                                 // (only the first n + 1 offsets are looked at)
    // longest_first: by decreasing length, equal lengths in index order
    const uint64_t lo[8] = {0, 4, 4, 8, 20, 24, 24, 36};        // lengths 4 0 4 12 4 0 12
    std::vector<uint32_t> ord(3, 99);
    longest_first(ord, lo, 7);
    const uint32_t want[7] = {3, 6, 0, 2, 4, 1, 5};
    CHECK(ord.size() == 7);
    for (size_t i = 0; i < 7; ++i) CHECK(ord[i] == want[i]);
    longest_first(ord, lo, 0);
    CHECK(ord.empty());
}

int main()
{
    CHECK(ensure_device() == ERR_OK);
    duplex_ok(16, 1, 4);
    duplex_ok(16, 1000, 64);
    duplex_ok(192, 777, 100);
    duplex_ok(16, 64 * 40, 64);
    for (int mode = 1; mode <= 3; ++mode) {
        duplex_fails(64 * 10, 64, 0, mode);
        duplex_fails(64 * 10, 64, 4, mode);
        duplex_fails(64 * 10 + 3, 64, 9, mode);
    }
    {   // several host threads, each with its own pipeline (streams are per thread)
        std::vector<std::thread> th;
        for (int t = 0; t < 4; ++t) th.emplace_back([t] { duplex_ok(16, 3000 + 100 * t, 128); });
        for (auto &t : th) t.join();
    }
    pool_and_fallback();
    stage_helper();
    ragged_part();
    worker_pool();
    CHECK(hipDeviceSynchronize() == hipSuccess);
    puts("staging mock ok");
    return 0;
}
