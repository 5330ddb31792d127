// needle_gather.h -- what needle_gather.hip's three kernels (needle_gather_spans_lengths_packed_dev / needle_gather_spans_fill_packed_dev /
// needle_split_spans_packed_dev) take: a packed batch and a CSR span list over its rows.  Pure functions of (text, list): no pattern.
//
// Unlike set_spans_kernel (needle_set_spans.h), where a lane owns a span and walks it alone, a span longer than a step of the fill kernel
// is copied by the WHOLE wave over several steps: the sweep is over output blocks, not over spans, so a 5000-unit span costs what 5000
// units of short spans cost.
#pragma once
#include <stdint.h>

namespace needle {

constexpr int kGatherWaves = 4;        // waves per workgroup; a wave owns a 64-row group at a time
constexpr uint32_t kGatherChunk = 256; // spans of a group per piece table (needle_gather_chunk_spans)

struct GatherArgs {
    const uint8_t *data;      // the rows' code units (device, 4-byte aligned)
    const uint64_t *in_off;   // n_rows + 1 row offsets, in code units
    uint64_t n_rows;
    uint32_t cw;              // 1 | 2
    const uint64_t *span_off; // n_rows + 1: row r's spans are start / end[span_off[r] .. span_off[r + 1])
    const int32_t *start, *end;
    uint64_t *out_len;        // lengths: indexed like start
    const uint64_t *out_off;  // fill: indexed like start, one entry more; in code units
    uint8_t *out;             // fill: the output code units (device, 4-byte aligned)
    uint64_t *piece_off;      // split: n_rows + 1
    int32_t *piece_start, *piece_end; // split: indexed by piece
};

} // namespace needle
