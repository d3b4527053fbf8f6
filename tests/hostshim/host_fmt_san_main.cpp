// TEST INFRASTRUCTURE: the host path of belt-fmt (bee2_amd/csrc/host_fmt.hpp) as a stand-alone program, so that
// tests/test_beltfmt.py can run it under -fsanitize=address,undefined as a subprocess of its own.  Reads cases from the file
// named by argv[1], one per line:   decr mod count key_len <key words, 8 hex> <iv hex | -> <count symbols>
// the first line being the 256 octets of the S-box in hex; writes each result as one line of symbols.  Nothing here ships.
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "../../bee2_amd/csrc/host_fmt.hpp"

using namespace bee2hip;
using namespace bee2hip::hostp;

static std::vector<uint8_t> unhex(const std::string &s)
{
    std::vector<uint8_t> out(s.size() / 2);
    for (size_t i = 0; i < out.size(); ++i) out[i] = (uint8_t)strtoul(s.substr(2 * i, 2).c_str(), nullptr, 16);
    return out;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    static char word[4096];
    if (fscanf(f, "%4095s", word) != 1) return 2;
    const std::vector<uint8_t> H = unhex(word);
    if (H.size() != 256) return 2;
    BeltTables T;
    belt_tables(T, H.data());
    int decr;
    unsigned mod;
    size_t count;
    while (fscanf(f, "%d %u %zu", &decr, &mod, &count) == 3) {
        uint32_t key[8];
        for (int k = 0; k < 8; ++k)
            if (fscanf(f, "%x", &key[k]) != 1) return 2;
        if (fscanf(f, "%4095s", word) != 1) return 2;
        const bool has_iv = word[0] != '-';
        const std::vector<uint8_t> iv = has_iv ? unhex(word) : std::vector<uint8_t>();
        if (has_iv && iv.size() != 16) return 2;
        std::vector<uint16_t> buf(count);                 // exactly the record: an access past it is the sanitizer's to find
        for (size_t i = 0; i < count; ++i) {
            unsigned v;
            if (fscanf(f, "%u", &v) != 1) return 2;
            buf[i] = (uint16_t)v;
        }
        fmt_crypt(T, decr, mod, count, key, H.data(), has_iv ? iv.data() : nullptr, buf.data());
        for (size_t i = 0; i < count; ++i) printf(i ? " %u" : "%u", (unsigned)buf[i]);
        printf("\n");
    }
    fclose(f);
    return 0;
}
