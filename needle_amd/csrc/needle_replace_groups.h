// needle_replace_groups.h -- what needle_replace_groups.hip's two kernels (needle_replace_groups_lengths_packed_dev /
// needle_replace_groups_fill_packed_dev) take: a packed batch, a CSR match list over its rows, the group planes of the matches and a
// parsed replacement template (needle_template.h).  Pure functions of (text, list, planes, template): no pattern.  The launch shape and
// the limit on the literals' code units are needle_replace.h's.
#pragma once
#include <stdint.h>

#include "needle_replace.h"

namespace needle {

constexpr uint32_t kTemplateMaxRefs = 16; // NEEDLE_TEMPLATE_MAX_REFS
// A replaced match is P pieces of output: its template's K group texts and non-empty literals (at most K + 1) in their order, then the
// gap of the input behind it.
constexpr uint32_t kGroupsMaxPieces = 2 * kTemplateMaxRefs + 2;
// Entries of a wave's piece table: 17 bytes a piece (O, D, the kind), and with 240 of them the fill kernel's LDS is 28 912 B -- five
// workgroups share a CU's 160 KiB as the replace-each kernel's do.  A chunk is floor(240 / P) matches: 60 for `$2-$1`, 7 at the most pieces.
constexpr uint32_t kGroupsTableEntries = 240;
// The template on the device, in front of the literals' units: words 0 .. 15 the K group numbers of the references (lengths kernel),
// words 16 .. 48 the P - 1 pieces of a replaced match in output order (fill kernel), whole 16 bytes.
//   a piece word: a group text  kGroupsRef | group number;  a literal  its byte offset among the literals | its bytes << 14.
constexpr uint32_t kGroupsHeadWords = 52;
constexpr uint32_t kGroupsHeadBytes = kGroupsHeadWords * 4;
constexpr uint32_t kGroupsPieceWord0 = 16;
constexpr uint32_t kGroupsRef = 0x80000000u;

struct ReplaceGroupsArgs {
    const uint8_t *data;       // the rows' code units (device, 4-byte aligned)
    const uint64_t *in_off;    // n_rows + 1 row offsets, in code units
    uint64_t n_rows;
    uint32_t cw;               // 1 | 2
    uint32_t n_refs;           // K: 0 .. kTemplateMaxRefs
    uint32_t lit_units;        // the literals' code units in all: <= kReplaceMaxUnits
    uint32_t pieces;           // P: 1 .. kGroupsMaxPieces
    uint32_t chunk;            // matches per piece table: kGroupsTableEntries / P
    uint32_t inv_pieces;       // ceil(65536 / P): k / P == (k * inv_pieces) >> 16 for k < kGroupsTableEntries (exact: 240 / 65536 < 1 / 34)
    const uint64_t *match_off; // n_rows + 1: row r's matches are columns match_off[r] .. match_off[r + 1] of the planes
    const int32_t *gstart, *gend; // plane g of match m at [g * plane_stride + m]; plane 0 the match itself, < 0: kept
    uint64_t plane_stride;
    const uint8_t *table;      // device, 16-byte aligned: kGroupsHeadBytes, then (fill only) lit_units * cw bytes, padded to whole 16 bytes
    uint64_t *out_len;         // lengths: n_rows
    const uint64_t *out_off;   // fill: n_rows + 1, in code units
    uint8_t *out;              // fill: the output code units (device, 4-byte aligned)
};

} // namespace needle
