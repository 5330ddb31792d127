// The device layout of a UTF-8 host chunk (needle_amd/csrc/needle_host_plan.h: utf8_chunk) on the CPU.  Reads lines "<rows> <text bytes>",
// prints per line the ten section offsets in the order they are laid out, then the total.
#include <cstdio>

#include "../../needle_amd/csrc/needle_host_plan.h"

int main() {
    unsigned long long nr, text;
    while (scanf("%llu %llu", &nr, &text) == 2) {
        needle::Slab lay;
        const needle::Utf8Chunk c = needle::utf8_chunk(lay, nr, text);
        printf("%llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)c.data, (unsigned long long)c.off, (unsigned long long)c.len,
               (unsigned long long)c.uoff, (unsigned long long)c.non_ascii, (unsigned long long)c.malformed, (unsigned long long)c.bitmap,
               (unsigned long long)c.cnt, (unsigned long long)c.csr, (unsigned long long)c.u16, (unsigned long long)lay.total());
    }
    return 0;
}
