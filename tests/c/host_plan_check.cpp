// needle_host_plan.h on the CPU (tests/test_host_plan.py builds this with -fsanitize=address,undefined): one case per line on stdin,
// one line of numbers per case on stdout.
//   stride ROW_STRIDE CHAR_WIDTH                              -> padded stride
//   fixed PADDED_STRIDE PER_ROW BUDGET                        -> rows per chunk
//   packed CHAR_WIDTH PER_ROW ALIGN BUDGET N off[0] .. off[N] -> r0 r1 of every chunk
//   csr R0 R1 MAX_M N off[0] .. off[N]                        -> a b of every range
//   class LEN_BYTES                                           -> length class
//   slab K bytes[0] .. bytes[K-1]                             -> the K offsets, then the total
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "../../needle_amd/csrc/needle_host_plan.h"

using namespace needle;

static std::vector<uint64_t> read_offsets() {
    uint64_t n = 0;
    std::cin >> n;
    std::vector<uint64_t> off(n + 1); // (exactly n + 1 entries: a planner that reads beyond them is the sanitizer's to report)
    for (uint64_t &o : off) std::cin >> o;
    return off;
}

static void print_ranges(const std::vector<RowRange> &rs) {
    for (const RowRange &r : rs) printf("%llu %llu ", (unsigned long long)r.first, (unsigned long long)r.second);
    printf("\n");
}

int main() {
    std::string what;
    while (std::cin >> what) {
        if (what == "stride") {
            uint64_t s, cw;
            std::cin >> s >> cw;
            printf("%llu\n", (unsigned long long)padded_stride_bytes(s, cw));
        } else if (what == "fixed") {
            uint64_t s, per_row, budget;
            std::cin >> s >> per_row >> budget;
            printf("%llu\n", (unsigned long long)fixed_chunk_rows(s, per_row, budget));
        } else if (what == "packed") {
            uint64_t cw, per_row, align, budget;
            std::cin >> cw >> per_row >> align >> budget;
            const std::vector<uint64_t> off = read_offsets();
            print_ranges(packed_chunks(off.data(), off.size() - 1, cw, per_row, align, budget));
        } else if (what == "csr") {
            uint64_t r0, r1, max_m;
            std::cin >> r0 >> r1 >> max_m;
            const std::vector<uint64_t> off = read_offsets();
            print_ranges(csr_ranges(off.data(), r0, r1, max_m));
        } else if (what == "class") {
            uint64_t b;
            std::cin >> b;
            printf("%d\n", length_class(b));
        } else if (what == "slab") {
            uint64_t k, b;
            std::cin >> k;
            Slab lay;
            for (uint64_t i = 0; i < k; ++i) {
                std::cin >> b;
                printf("%llu ", (unsigned long long)lay.add(b));
            }
            printf("%llu\n", (unsigned long long)lay.total());
        } else {
            fprintf(stderr, "unknown case %s\n", what.c_str());
            return 2;
        }
    }
    return 0;
}
