// The arithmetic of the host-buffer entries (needle_host.cpp): how a host batch is cut into chunks that keep a bounded amount resident on
// the device, and where the sections of a chunk lie in its one device buffer.  Pure host code -- no HIP, no global state, the budgets are
// arguments -- so that tests/c/host_plan_check.cpp runs it on the CPU under a sanitizer.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <utility>
#include <vector>

namespace needle {

inline uint64_t up16(uint64_t x) { return (x + 15) & ~(uint64_t)15; }

// The stride of a fixed-stride host row on the device: whole 16 bytes, at least 16.
inline uint64_t padded_stride_bytes(uint64_t row_stride, uint64_t char_width) { return std::max<uint64_t>(16, up16(row_stride * char_width)); }

// Rows per chunk of a fixed-stride host batch: a row costs its padded text + per_row bytes on the device; whole 64-row groups (every
// chunk owns whole bitmap words), at least one.
inline uint64_t fixed_chunk_rows(uint64_t padded_stride, uint64_t per_row, uint64_t budget) {
    return std::max<uint64_t>(64, (budget / (padded_stride + per_row)) & ~(uint64_t)63);
}

using RowRange = std::pair<uint64_t, uint64_t>; // rows [first, second)

// The chunks of a packed host batch (offsets: n_rows + 1 entries, non-decreasing; offsets[0] may be > 0): consecutive rows, at least
// `align` rows (or the rest), grown `align` rows at a time while the chunk's text + per_row bytes per row stay within the budget.
inline std::vector<RowRange> packed_chunks(const uint64_t *offsets, uint64_t n_rows, uint64_t char_width, uint64_t per_row, uint64_t align,
                                           uint64_t budget) {
    auto cost = [&](uint64_t r0, uint64_t r1) { return (offsets[r1] - offsets[r0]) * char_width + (r1 - r0) * per_row; };
    std::vector<RowRange> chunks;
    for (uint64_t r0 = 0; r0 < n_rows;) {
        uint64_t r1 = std::min<uint64_t>(r0 + align, n_rows);
        while (r1 < n_rows && cost(r0, std::min<uint64_t>(r1 + align, n_rows)) <= budget) r1 = std::min<uint64_t>(r1 + align, n_rows);
        chunks.emplace_back(r0, r1);
        r0 = r1;
    }
    return chunks;
}

// Device bytes of one match of a CSR fill pass: int32 start + end, and a uint32 mask beside them where the matches are tagged by a
// pattern set (needle_set_tag_matches_packed_host).
inline uint64_t csr_match_bytes(bool tagged) { return tagged ? 12 : 8; }

// The row ranges of a CSR fill pass over rows [r0, r1), whose match counts stand summed up in `offsets`: at least one row each, at most
// max_m matches (one row may exceed it).
inline std::vector<RowRange> csr_ranges(const uint64_t *offsets, uint64_t r0, uint64_t r1, uint64_t max_m) {
    std::vector<RowRange> ranges;
    for (uint64_t a = r0; a < r1;) {
        uint64_t b = a + 1;
        while (b < r1 && offsets[b + 1] - offsets[a] <= max_m) ++b;
        ranges.emplace_back(a, b);
        a = b;
    }
    return ranges;
}

// The length class of a packed row that goes to the kernels as a fixed-stride one: the smallest k with len_bytes <= 64 << 2k (strides of
// 64 B, 256 B, 1 KiB, ... x4: the padded bytes of a class stay below 4x its text).  len_bytes < 2^62.
inline int length_class(uint64_t len_bytes) {
    int k = 0;
    while (len_bytes > (64ull << (2 * k))) ++k;
    return k;
}

// The sections of one device buffer: add(bytes) is the next section's offset, a multiple of 16; total() the bytes to allocate.
struct Slab {
    uint64_t end = 0;
    uint64_t add(uint64_t bytes) {
        const uint64_t at = up16(end);
        end = at + bytes;
        return at;
    }
    uint64_t total() const { return end; }
};

// One chunk of a UTF-8 packed host batch on the device (needle_*_utf8_packed_host): the text | its nr + 1 row offsets | the units of every
// row | the nr + 1 unit offsets | the non-ASCII and malformed bitmaps | the results -- containedIn's bitmap, or find-all's counts and its
// fill pass's offsets -- | the UTF-16 text.  units(row) <= bytes(row) (NEEDLE_UTF8_MAX_EXPANSION), so the UTF-16 form never needs more
// than 2 bytes per byte of text: the chunk reserves text + 2 * text + the lists, whatever the rows hold.
struct Utf8Chunk {
    uint64_t data, off, len, uoff, non_ascii, malformed, bitmap, cnt, csr, u16;
};
constexpr uint64_t kUtf8RowBytes = 8 + 8 + 8 + 4 + 8 + 1; // what a row costs beside its text: offsets, units, unit offsets, count, csr, bitmaps
inline Utf8Chunk utf8_chunk(Slab &lay, uint64_t nr, uint64_t text_bytes) {
    const uint64_t words = (nr + 63) / 64 * 8;
    Utf8Chunk c;
    c.data = lay.add(std::max<uint64_t>(text_bytes, 4));
    c.off = lay.add((nr + 1) * 8);
    c.len = lay.add(nr * 8);
    c.uoff = lay.add((nr + 1) * 8);
    c.non_ascii = lay.add(words);
    c.malformed = lay.add(words);
    c.bitmap = lay.add(words);
    c.cnt = lay.add(nr * 4);
    c.csr = lay.add((nr + 1) * 8);
    c.u16 = lay.add(std::max<uint64_t>(2 * text_bytes, 4));
    return c;
}

} // namespace needle
