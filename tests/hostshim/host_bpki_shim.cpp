// TEST INFRASTRUCTURE: a C view of bee2_amd/csrc/bpki_der.hpp -- the parser and builder of the bpki container frames -- for
// tests/test_bpki.py, and a program of its own for a sanitizer build:
//   g++ -O2 -shared -fPIC                      -> the library the test loads (hb_* below)
//   g++ -O1 -g -fsanitize=address,undefined -static-libasan -static-libubsan
//                                              -> a program: `host_bpki_shim corpus.txt` reads one container per line as hex (an
//     empty line is the empty container), runs both parsers over each from a heap block of exactly its size, rebuilds what was
//     accepted and compares, then does the same over 10 000 seeded one-octet mutations and truncations of the first line.
//     Exit 0 and no report: every read stayed inside its input.  The runtimes are linked statically: the program runs in any
//     environment as it is.  Nothing here ships.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../bee2_amd/csrc/bpki_der.hpp"

using namespace bee2hip::bpki;

extern "C" {
// -> 1 when accepted, with salt[8], *iter, *off and *len of encData
int hb_epki_parse(const uint8_t *epki, size_t n, uint8_t salt[8], uint64_t *iter, size_t *off, size_t *len)
{
    const Epki e = epki_parse(epki, n);
    if (!e.ok) return 0;
    memcpy(salt, e.salt, 8);
    *iter = e.iter; *off = e.edata_off; *len = e.edata_len;
    return 1;
}
// -> the key's length (0: refused), key[64]
size_t hb_pki_parse(int kind, const uint8_t *pki, size_t n, uint8_t key[64]) { return pki_parse(kind, pki, n, key); }
size_t hb_pki_build(uint8_t *out, int kind, const uint8_t *key, size_t key_len) { return pki_build(out, kind, key, key_len); }
size_t hb_epki_build(uint8_t *out, const uint8_t salt[8], uint64_t iter, const uint8_t *edata, size_t edata_len)
{
    return epki_build(out, salt, iter, edata, edata_len, nullptr);
}
}

// ---- the program
static unsigned long g_accepted = 0, g_inner = 0;
static int fail(const char *what, size_t n)
{
    fprintf(stderr, "host_bpki_shim: %s (input of %zu octets)\n", what, n);
    return 1;
}
// one input, from a heap block of exactly n octets
static int one(const uint8_t *data, size_t n)
{
    uint8_t *p = (uint8_t *)malloc(n ? n : 1);
    if (!p) return fail("out of memory", n);
    if (n) memcpy(p, data, n);
    int bad = 0;
    const Epki e = epki_parse(n ? p : nullptr, n);
    if (e.ok) {
        ++g_accepted;
        if (e.edata_off > n || e.edata_len > n - e.edata_off) bad = fail("encData outside the container", n);
        else if (e.iter != 0) {
            // (bee2 takes an INTEGER of no octets for 0, which no builder writes: only a nonzero count is rebuilt)
            const size_t want = epki_build(nullptr, e.salt, e.iter, nullptr, e.edata_len, nullptr);
            uint8_t *q = (uint8_t *)malloc(want);
            if (!q || epki_build(q, e.salt, e.iter, p + e.edata_off, e.edata_len, nullptr) != want) bad = fail("builder length", n);
            // the only accepted frames that differ from the rebuilt one carry octets of an unfinished arc behind an OID
            else if (want == n && memcmp(p, q, n) != 0) bad = fail("an accepted frame of the rebuilt length differs from it", n);
            else if (want > n) bad = fail("an accepted frame is shorter than the rebuilt one", n);
            free(q);
        }
    }
    for (int kind = 0; kind < 2 && !bad; ++kind) {
        uint8_t key[KEY_MAX], again[KEY_MAX + 64];
        const size_t len = pki_parse(kind, n ? p : nullptr, n, key);
        if (len) {
            ++g_inner;
            const size_t m = pki_build(again, kind, key, len);
            // (bee2 accepts a version INTEGER of no octets and an unfinished arc behind an OID: those are not what is rebuilt)
            if (m == n && memcmp(again, p, n) != 0) bad = fail("an accepted inner frame of the rebuilt length differs from it", n);
        }
    }
    free(p);
    return bad;
}

static int hexval(int c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s corpus.txt\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    static char line[1 << 16];
    static uint8_t buf[1 << 15], first[1 << 15];
    size_t first_n = 0, lines = 0;
    while (fgets(line, sizeof line, f)) {
        size_t n = 0;
        for (const char *c = line; hexval(c[0]) >= 0 && hexval(c[1]) >= 0; c += 2) buf[n++] = (uint8_t)(hexval(c[0]) << 4 | hexval(c[1]));
        if (lines++ == 0) { memcpy(first, buf, n); first_n = n; }
        if (one(buf, n)) return 1;
    }
    fclose(f);
    if (first_n == 0) { fprintf(stderr, "host_bpki_shim: the first line must hold a container\n"); return 2; }
    uint64_t z = 0x9E3779B97F4A7C15ull;
    for (int it = 0; it < 10000; ++it) {
        z ^= z << 13; z ^= z >> 7; z ^= z << 17;
        memcpy(buf, first, first_n);
        size_t n = first_n;
        buf[(z >> 8) % first_n] = (uint8_t)(z >> 40);
        if (it % 4 == 3) n = (z >> 24) % (first_n + 1);                 // and every fourth is cut as well
        if (one(buf, n)) return 1;
    }
    printf("host_bpki_shim: %zu lines + 10000 mutations; %lu outer and %lu inner frames accepted\n", lines, g_accepted, g_inner);
    return 0;
}
