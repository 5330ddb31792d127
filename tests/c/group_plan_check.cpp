// needle_group.h's workspace layout on the CPU (tests/test_group_abi.py builds this with -fsanitize=address,undefined): one case per line
// on stdin, one line of numbers per case on stdout.
//   layout MAX_SPANS   -> slots addr hash slot len word count clear_at clear_bytes total
//   mask HASH_BITS     -> the hash mask
//   touch MAX_SPANS    -> 1: a buffer of exactly `total` bytes takes a write to the first and last entry of every section (the
//                         sanitizer reports one that lies outside)
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../needle_amd/csrc/needle_group.h"

using namespace needle;

int main() {
    std::string what;
    while (std::cin >> what) {
        unsigned long long x = 0;
        std::cin >> x;
        if (what == "layout") {
            const GroupLayout g = group_layout(x);
            const unsigned long long v[] = {g.slots, g.addr, g.hash, g.slot, g.len, g.word, g.count, g.clear_at, g.clear_bytes, g.total};
            for (unsigned long long n : v) printf("%llu ", n);
            printf("\n");
        } else if (what == "mask") {
            printf("%llu\n", (unsigned long long)group_hash_mask((uint32_t)x));
        } else if (what == "touch") {
            const GroupLayout g = group_layout(x);
            std::vector<uint8_t> buf(g.total);
            auto put = [&](uint64_t at, uint64_t entries, uint64_t size) {
                if (!entries) return;
                memset(buf.data() + at, 0xA5, size);
                memset(buf.data() + at + (entries - 1) * size, 0xA5, size);
            };
            put(g.addr, x, 8), put(g.hash, x, 8), put(g.slot, x, 8), put(g.len, x, 4), put(g.word, g.slots, 4), put(g.count, g.slots, 4);
            memset(buf.data() + g.clear_at, 0, g.clear_bytes);
            printf("1\n");
        } else {
            return 2;
        }
    }
    return 0;
}
