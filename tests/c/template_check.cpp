// The template parser (needle_amd/csrc/needle_template.h) as a stand-alone program for tests/test_replace_groups_abi.py, which builds it
// with -fsanitize=address,undefined.  stdin: one template per line, "G n u_0 .. u_(n-1)" (UTF-16 code units in decimal).
// stdout: per line "E" for an error, else "K g_1 .. g_K off_0 .. off_(K+1) lits...".
#include <cstdio>
#include <string>
#include <vector>

#include "../../needle_amd/csrc/needle_template.h"

int main() {
    unsigned long G, n;
    while (scanf("%lu %lu", &G, &n) == 2) {
        std::vector<uint16_t> t(n); // (exactly n units: a read behind the template is a heap overflow the sanitizer sees)
        for (auto &u : t) {
            unsigned v;
            if (scanf("%u", &v) != 1) return 2;
            u = (uint16_t)v;
        }
        needle::TemplateForm f;
        std::string err;
        if (!needle::template_parse(t.data(), t.size(), (uint32_t)G, &f, &err)) {
            if (err.empty()) return 3;
            puts("E");
            continue;
        }
        if (f.lit_offsets.size() != f.groups.size() + 2 || f.lit_offsets.front() != 0 || f.lit_offsets.back() != f.lits.size()) return 4;
        printf("%zu", f.groups.size());
        for (int32_t g : f.groups) printf(" %d", g);
        for (uint32_t o : f.lit_offsets) printf(" %u", o);
        for (uint16_t u : f.lits) printf(" %u", (unsigned)u);
        putchar('\n');
    }
    return 0;
}
