// needle_utf8.h -- UTF-8 packed rows in front of the UTF-16 kernels (needle_utf16_lengths_from_utf8_packed_dev,
// needle_utf16_from_utf8_packed_dev, needle_utf8_positions_packed_dev; include/needle_hip.h): THE rule -- which bytes of a
// row start a UTF-16 unit, which of them file two, which file U+FFFD -- stated once, as a function over one aligned 16-byte block that
// needle_utf8.hip's three kernels call.  The function is plain C++ (host and device), so that tests/c/utf8_classify_check.cpp runs it
// on the CPU against the byte-by-byte statement of the rule.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NEEDLE_UTF8_HD __host__ __device__ __forceinline__
#define NEEDLE_UTF8_UNROLL _Pragma("unroll")
#else
#define NEEDLE_UTF8_HD inline
#define NEEDLE_UTF8_UNROLL
#endif

namespace needle {

// What a 16-byte block files, one bit per byte of the block (bit j: the block's byte j).
struct Utf8Masks {
    uint32_t starts; // the byte starts a unit (it is not consumed by a sequence that began before it)
    uint32_t pairs;  // ... and files a surrogate pair: the lead of a complete 4-byte sequence
    uint32_t bad;    // ... and files U+FFFD
    uint32_t high;   // the byte is >= 0x80
};

// ---- the rule (Unicode s3.9, "maximal subpart"; the JDK's and CPython's decoders), on four bytes per dword.
// A mask holds bit 7 of every byte for which its predicate holds.  need(b): 2 for C2..DF, 3 for E0..EF, 4 for F0..F4, else 0;
// second_ok(l, b): b in A0..BF for l = E0, 80..9F for ED, 90..BF for F0, 80..8F for F4, 80..BF otherwise; cont(b): b in 80..BF.
//   byte i is CONSUMED iff cont(b[i]) and one of
//     need(b[i-1]) >= 2 && second_ok(b[i-1], b[i]);   need(b[i-2]) >= 3 && second_ok(b[i-2], b[i-1]);
//     need(b[i-3]) == 4 && second_ok(b[i-3], b[i-2]) && cont(b[i-1])
//   with every byte named in the SAME ROW as byte i; every other byte is a START and files: itself below 0x80; the code point (two units
//   for k == 4) if k = need(b[i]) > 0, second_ok(b[i], b[i+1]) and b[i+2 .. i+k-1] are continuation bytes of the same row; else U+FFFD.
// The window is six dwords: the dword before the block (its bytes 1..3 are the three bytes before the block; byte 0 is ignored), the
// block, the dword behind it (bytes 0..2; byte 3 is ignored).  Bytes outside the batch are ZERO when they get here: a zero byte neither
// continues nor begins a sequence.  Rows inside the window are told apart by `first24`: bit k says that byte k of the window (k = 4 is the
// block's first byte) is the first byte of a row -- a block of short rows holds several.  ONE_ROW: the caller has zeroed every byte of
// another row, first24 is not looked at.
namespace utf8_detail {
constexpr uint32_t kB7 = 0x80808080u;
// bit 7 of every byte whose low seven bits are >= k (k in 1 .. 0x80); y holds the low seven bits, so no carry leaves a byte
NEEDLE_UTF8_HD uint32_t ge7(uint32_t y, uint32_t k) { return y + (0x80u - k) * 0x01010101u; }
// four bits -> bit 7 of four bytes
NEEDLE_UTF8_HD uint32_t spread4(uint32_t nib) { return (((nib & 0xFu) * 0x00204081u) & 0x01010101u) << 7; }
// bit 7 of four bytes -> four bits
NEEDLE_UTF8_HD uint32_t gather4(uint32_t m) { return (((m >> 7) & 0x01010101u) * 0x00204081u >> 21) & 0xFu; }
// byte i of the result is byte i - K of the window (up) / byte i + K (down); zeros come in at the window's ends
template <int K>
NEEDLE_UTF8_HD uint32_t up(const uint32_t *m, int d) { return (m[d] << (8 * K)) | (d > 0 ? m[d - 1] >> (32 - 8 * K) : 0u); }
template <int K>
NEEDLE_UTF8_HD uint32_t down(const uint32_t *m, int d) { return (m[d] >> (8 * K)) | (d < 5 ? m[d + 1] << (32 - 8 * K) : 0u); }
} // namespace utf8_detail

template <bool ONE_ROW>
NEEDLE_UTF8_HD Utf8Masks utf8_classify16(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3, uint32_t before, uint32_t after, uint32_t first24) {
    using namespace utf8_detail;
    const uint32_t w[6] = {before & 0xFFFFFF00u, b0, b1, b2, b3, after & 0x00FFFFFFu};
    uint32_t H[6], L2[6], L3[6], L4[6], is2[6], is3[6], A[6], B[6], C[6], X1[6], X2[6], X3[6], cont[6], G[6], Sp[6];
    NEEDLE_UTF8_UNROLL
    for (int d = 0; d < 6; ++d) {
        const uint32_t h = w[d] & kB7, y = w[d] & 0x7F7F7F7Fu;
        const uint32_t g10 = ge7(y, 0x10) & h, g20 = ge7(y, 0x20) & h, g40 = ge7(y, 0x40) & h, g42 = ge7(y, 0x42) & h;
        const uint32_t g60 = ge7(y, 0x60) & h, g61 = ge7(y, 0x61) & h, g6D = ge7(y, 0x6D) & h, g6E = ge7(y, 0x6E) & h;
        const uint32_t g70 = ge7(y, 0x70) & h, g71 = ge7(y, 0x71) & h, g74 = ge7(y, 0x74) & h, g75 = ge7(y, 0x75) & h;
        H[d] = h;
        cont[d] = h & ~g40;                                        // 80..BF
        A[d] = h & ~g10, B[d] = g10 & ~g20, C[d] = g20 & ~g40;     // 80..8F, 90..9F, A0..BF
        is2[d] = g42 & ~g60, is3[d] = g60 & ~g70, L4[d] = g70 & ~g75; // need == 2, 3, 4
        L2[d] = g42 & ~g75, L3[d] = g60 & ~g75;                    // need >= 2, >= 3
        const uint32_t e0 = g60 & ~g61, ed = g6D & ~g6E, f0 = g70 & ~g71, f4 = g74 & ~g75;
        X1[d] = e0 | f0, X2[d] = e0 | f4, X3[d] = ed | f4;         // the leads whose second byte must not be in A, in B, in C
    }
    NEEDLE_UTF8_UNROLL
    for (int d = 0; d < 6; ++d) {
        const uint32_t nf = ONE_ROW ? kB7 : spread4(~first24 >> (4 * d)); // the byte is in the row of the byte before it
        const uint32_t second = cont[d] & ~((up<1>(X1, d) & A[d]) | (up<1>(X2, d) & B[d]) | (up<1>(X3, d) & C[d])); // second_ok(b[i-1], b[i])
        Sp[d] = second & nf;
        G[d] = cont[d] & nf;
    }
    Utf8Masks m = {0u, 0u, 0u, 0u};
    NEEDLE_UTF8_UNROLL
    for (int d = 1; d < 5; ++d) {
        const uint32_t consumed = (up<1>(L2, d) & Sp[d]) | (up<2>(L3, d) & up<1>(Sp, d) & G[d]) | (up<3>(L4, d) & up<2>(Sp, d) & up<1>(G, d) & G[d]);
        const uint32_t c2 = down<1>(Sp, d), c3 = c2 & down<2>(G, d), c4 = c3 & down<3>(G, d);
        const uint32_t complete = (is2[d] & c2) | (is3[d] & c3) | (L4[d] & c4);
        const uint32_t start = ~consumed & kB7;
        const int at = 4 * (d - 1);
        m.starts |= gather4(start) << at;
        m.pairs |= gather4(L4[d] & c4) << at;
        m.bad |= gather4(start & H[d] & ~complete) << at;
        m.high |= gather4(H[d]) << at;
    }
    return m;
}

// The unit(s) a start files, from the four bytes at the start (q: the start's byte in bits 0..7, the next ones above it), given its
// verdict: bad -> U+FFFD; else the byte below 0x80, or the code point of the sequence its lead announces (pair: the high surrogate,
// *low the low one).
NEEDLE_UTF8_HD uint32_t utf8_unit(uint32_t q, bool bad, uint32_t *low) {
    const uint32_t c0 = q & 0xFFu, c1 = (q >> 8) & 0x3Fu, c2 = (q >> 16) & 0x3Fu, c3 = (q >> 24) & 0x3Fu;
    *low = 0u;
    if (bad) return 0xFFFDu;
    if (c0 < 0x80u) return c0;
    if (c0 < 0xE0u) return ((c0 & 0x1Fu) << 6) | c1;
    if (c0 < 0xF0u) return ((c0 & 0x0Fu) << 12) | (c1 << 6) | c2;
    const uint32_t cp = (((c0 & 0x07u) << 18) | (c1 << 12) | (c2 << 6) | c3) - 0x10000u;
    *low = 0xDC00u | (cp & 0x3FFu);
    return 0xD800u | (cp >> 10);
}

} // namespace needle
