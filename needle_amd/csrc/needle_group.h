// needle_group.h -- what needle_group.hip's three kernels (needle_group_spans_packed_dev) take, and where the sections of
// the caller's workspace lie.  No HIP in here: the layout is plain arithmetic (needle_host_plan.h's Slab), so that
// tests/c/group_plan_check.cpp runs it on the CPU under a sanitizer.
//
// Equal spans of a CSR list over packed rows are put into groups: per span the first span with the same text and the size of its group.
// A pure function of (text, list), like the gather: no pattern.
//   Pass 1 (hash):   a wave owns a 64-row group, lanes are spans; per span the absolute byte address of its clamped start, its length
//                    in bytes (kGroupAbsent: an absent span) and a 64-bit hash of (text, length), masked to hash_bits.
//   Pass 2 (insert): a lane is a span; open addressing with linear probing over `slots` 32-bit words holding rep + 1 (rep relative
//                    to M0; 0: empty), one compare-and-swap per empty slot seen, text compared against the occupant's, an unsigned
//                    min turns the representative into the first occurrence, a count per slot.
//   Pass 3 (finish): d_first[m] = M0 + word[slot[m]] - 1, d_count[m] = count[slot[m]].
// Stream order is the only barrier between the passes.
#pragma once
#include <stdint.h>

#include "needle_host_plan.h"

namespace needle {

constexpr int kGroupWaves = 4;                   // waves per workgroup
constexpr uint64_t kGroupMaxSpans = 0xFFFFFFFEull; // rep + 1 fits the 32-bit slot word
constexpr uint32_t kGroupAbsent = 0xFFFFFFFFu;   // in the length array (a row has at most 2^31 - 1 units: 2^32 - 2 bytes)
constexpr uint64_t kGroupNoSlot = ~0ull;         // in the slot array: the probe found no slot (status 1)
constexpr uint64_t kGroupMinSlots = 64;

// The table's slots: the smallest power of two >= 2 * max_spans, at least kGroupMinSlots (max_spans <= kGroupMaxSpans: at most 2^33).
inline uint64_t group_slots(uint64_t max_spans) {
    uint64_t s = kGroupMinSlots;
    while (s < 2 * max_spans) s <<= 1;
    return s;
}

// The hash's bits that are used: the low hash_bits (0 .. 64).
inline uint64_t group_hash_mask(uint32_t hash_bits) { return hash_bits >= 64 ? ~0ull : (1ull << hash_bits) - 1; }

// The workspace (16-byte aligned sections; the caller's pointer is 16-byte aligned): per span its address, masked hash and slot (8 bytes
// each) and its length (4), then the table -- the slot words and, right behind them, the slot counts: ONE range to clear.
struct GroupLayout {
    uint64_t slots;
    uint64_t addr, hash, slot, len; // per span: max_spans entries each
    uint64_t word, count;           // per slot: uint32 each; count = word + 4 * slots
    uint64_t clear_at, clear_bytes; // what the entry clears before pass 1: the table
    uint64_t total;
};

inline GroupLayout group_layout(uint64_t max_spans) {
    GroupLayout g;
    Slab lay;
    g.slots = group_slots(max_spans);
    g.addr = lay.add(max_spans * 8);
    g.hash = lay.add(max_spans * 8);
    g.slot = lay.add(max_spans * 8);
    g.len = lay.add(max_spans * 4);
    g.word = lay.add(g.slots * 4);
    g.count = lay.add(g.slots * 4); // (slots * 4 is a multiple of 16: no gap)
    g.clear_at = g.word;
    g.clear_bytes = g.slots * 8;
    g.total = up16(lay.total());
    return g;
}

struct GroupArgs {
    const uint8_t *data;      // the rows' code units (device, 4-byte aligned)
    const uint64_t *in_off;   // n_rows + 1 row offsets, in code units
    uint64_t n_rows;
    uint32_t cw;              // 1 | 2
    const uint64_t *span_off; // n_rows + 1: row r's spans are start / end[span_off[r] .. span_off[r + 1])
    const int32_t *start, *end;
    uint64_t max_spans;       // the caller's bound on span_off[n_rows] - span_off[0]
    uint64_t hash_mask;
    uint64_t slots;           // a power of two
    uint64_t *w_addr, *w_hash, *w_slot; // the workspace's sections
    uint32_t *w_len, *w_word, *w_count;
    uint64_t *first;          // indexed like start
    uint32_t *count;          // indexed like start
    uint32_t *status;
};

} // namespace needle
