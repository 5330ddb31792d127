// The one statement of the UTF-8 rule the kernels use (needle_amd/csrc/needle_utf8.h: utf8_classify16, four bytes per dword) against the
// byte-by-byte statement of the same rule, on the CPU: seeded windows of 22 bytes with random row boundaries.  Prints "ok <cases>".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../needle_amd/csrc/needle_utf8.h"

static int need(uint8_t b) { return b >= 0xC2 && b <= 0xDF ? 2 : b >= 0xE0 && b <= 0xEF ? 3 : b >= 0xF0 && b <= 0xF4 ? 4 : 0; }
static bool cont(uint8_t b) { return b >= 0x80 && b <= 0xBF; }
static bool second_ok(uint8_t l, uint8_t b) {
    if (l == 0xE0) return b >= 0xA0 && b <= 0xBF;
    if (l == 0xED) return b >= 0x80 && b <= 0x9F;
    if (l == 0xF0) return b >= 0x90 && b <= 0xBF;
    if (l == 0xF4) return b >= 0x80 && b <= 0x8F;
    return cont(b);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

static const uint8_t kAlphabet[25] = {0x00, 0x41, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF,
                                      0xE0, 0xE1, 0xEC, 0xED, 0xEE, 0xEF, 0xF0, 0xF1, 0xF3, 0xF4, 0xF5, 0xFF};

int main() {
    uint64_t cases = 0;
    for (int it = 0; it < 3000000; ++it) {
        // window bytes 0..23: 4..19 are the block; 1..3 and 20..22 are what the rule may look at; 0 and 23 must be ignored
        uint8_t win[24];
        const uint32_t kind = rnd() % 3;
        for (int i = 0; i < 24; ++i) win[i] = kind == 0 ? (uint8_t)rnd() : kind == 1 ? kAlphabet[rnd() % 25] : (rnd() % 4 ? kAlphabet[3 + rnd() % 22] : (uint8_t)'a');
        uint32_t first = 0;
        const uint32_t density = rnd() % 4; // 0: one row
        for (int i = 0; i < 24; ++i)
            if (density && rnd() % (1u << (2 * density)) == 0) first |= 1u << i;
        const bool one_row = density == 0;
        int row[24];
        row[0] = 0;
        for (int i = 1; i < 24; ++i) row[i] = row[i - 1] + ((first >> i) & 1);
        uint32_t starts = 0, pairs = 0, bad = 0, high = 0;
        for (int j = 0; j < 16; ++j) {
            const int i = j + 4;
            auto same = [&](int k) { return k >= 1 && k <= 22 && row[k] == row[i]; }; // (bytes 0 and 23 are not part of the window)
            const uint8_t b = win[i];
            bool consumed = false;
            if (cont(b)) {
                consumed |= same(i - 1) && need(win[i - 1]) >= 2 && second_ok(win[i - 1], b);
                consumed |= same(i - 2) && need(win[i - 2]) >= 3 && second_ok(win[i - 2], win[i - 1]);
                consumed |= same(i - 3) && need(win[i - 3]) == 4 && second_ok(win[i - 3], win[i - 2]) && cont(win[i - 1]);
            }
            if (b >= 0x80) high |= 1u << j;
            if (consumed) continue;
            starts |= 1u << j;
            if (b < 0x80) continue;
            const int k = need(b);
            bool complete = k > 0 && same(i + k - 1) && second_ok(b, win[i + 1]);
            for (int t = 2; complete && t < k; ++t) complete = cont(win[i + t]);
            if (!complete) bad |= 1u << j;
            else if (k == 4) pairs |= 1u << j;
        }
        uint32_t w[6];
        memcpy(w, win, 24);
        const needle::Utf8Masks m = one_row ? needle::utf8_classify16<true>(w[1], w[2], w[3], w[4], w[0], w[5], 0xFFFFFFu)
                                            : needle::utf8_classify16<false>(w[1], w[2], w[3], w[4], w[0], w[5], first);
        if (m.starts != starts || m.pairs != pairs || m.bad != bad || m.high != high) {
            fprintf(stderr, "case %d: got %04x %04x %04x %04x, rule %04x %04x %04x %04x, first %06x, bytes", it, m.starts, m.pairs, m.bad, m.high, starts, pairs,
                    bad, high, first);
            for (int i = 0; i < 24; ++i) fprintf(stderr, " %02x", win[i]);
            fprintf(stderr, "\n");
            return 1;
        }
        ++cases;
    }
    // the units of every complete sequence: every code point through its UTF-8 form
    for (uint32_t cp = 0; cp < 0x110000u; ++cp) {
        if (cp >= 0xD800u && cp < 0xE000u) continue;
        uint32_t q;
        if (cp < 0x80u) q = cp;
        else if (cp < 0x800u) q = (0xC0u | (cp >> 6)) | (0x80u | (cp & 0x3Fu)) << 8;
        else if (cp < 0x10000u) q = (0xE0u | (cp >> 12)) | (0x80u | ((cp >> 6) & 0x3Fu)) << 8 | (0x80u | (cp & 0x3Fu)) << 16;
        else q = (0xF0u | (cp >> 18)) | (0x80u | ((cp >> 12) & 0x3Fu)) << 8 | (0x80u | ((cp >> 6) & 0x3Fu)) << 16 | (0x80u | (cp & 0x3Fu)) << 24;
        q |= cp < 0x80u ? 0xABCDEF00u : cp < 0x800u ? 0xABCD0000u : cp < 0x10000u ? 0xAB000000u : 0u; // the bytes of what follows: not looked at
        uint32_t low = 7;
        const uint32_t u = needle::utf8_unit(q, false, &low);
        const uint32_t want = cp < 0x10000u ? cp : 0xD800u + ((cp - 0x10000u) >> 10), want_low = cp < 0x10000u ? 0u : 0xDC00u + ((cp - 0x10000u) & 0x3FFu);
        if (u != want || low != want_low) {
            fprintf(stderr, "U+%04X: got %04x %04x\n", cp, u, low);
            return 1;
        }
        ++cases;
    }
    uint32_t low = 7;
    if (needle::utf8_unit(0x808080F0u, true, &low) != 0xFFFDu || low != 0u) return 1;
    printf("ok %llu\n", (unsigned long long)cases);
    return 0;
}
