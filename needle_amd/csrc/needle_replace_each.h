// needle_replace_each.h -- what needle_replace_each.hip's two kernels (needle_replace_each_lengths_packed_dev /
// needle_replace_each_fill_packed_dev) take: a packed batch, a CSR match list over its rows, a choice per match and a table of literal
// replacements.  Pure functions of (text, list, choices, table): no pattern.  The launch shape and the limit on the table's code units
// are needle_replace.h's.
#pragma once
#include <stdint.h>

#include "needle_replace.h"

namespace needle {

constexpr uint32_t kReplaceMaxChoices = 256;                              // NEEDLE_REPLACE_MAX_CHOICES
// Matches of a group per piece table: 20 bytes a piece here (O, D and the replacement's place), and with 240 of them the fill kernel's
// LDS is 32 624 B -- five workgroups share a CU's 160 KiB as the plain kernel's do (with kReplaceChunk it is 33 904 B: four).
constexpr uint32_t kReplaceEachChunk = 240;
constexpr uint32_t kReplaceEachOffsetBytes = (kReplaceMaxChoices + 4) * 4; // the table's n_repl + 1 offsets in front of its units, whole 16 bytes

struct ReplaceEachArgs {
    const uint8_t *data;       // the rows' code units (device, 4-byte aligned)
    const uint64_t *in_off;    // n_rows + 1 row offsets, in code units
    uint64_t n_rows;
    uint32_t cw;               // 1 | 2
    uint32_t n_repl;           // 1 .. kReplaceMaxChoices
    uint32_t choice_form;      // 0: int32 index, 1: uint32 mask, the index is its lowest set bit
    uint32_t table_units;      // the table's code units in all: <= kReplaceMaxUnits
    const uint64_t *match_off; // n_rows + 1: row r's matches are start / end / choice[match_off[r] .. match_off[r + 1])
    const int32_t *start, *end;
    const uint32_t *choice;
    const uint8_t *table;      // device, 16-byte aligned: kReplaceEachOffsetBytes of uint32 offsets in code units (entries behind n_repl: 0), then
                               // (fill only) table_units * cw bytes, padded to whole 16 bytes
    uint64_t *out_len;         // lengths: n_rows
    const uint64_t *out_off;   // fill: n_rows + 1, in code units
    uint8_t *out;              // fill: the output code units (device, 4-byte aligned)
};

} // namespace needle
