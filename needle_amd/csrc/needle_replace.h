// needle_replace.h -- what needle_replace.hip's two kernels (needle_replace_all_lengths_packed_dev / needle_replace_all_fill_packed_dev)
// take: a packed batch, a CSR match list over its rows, a literal replacement.  Pure functions of (text, list, replacement): no pattern.
#pragma once
#include <stdint.h>

namespace needle {

constexpr uint32_t kReplaceMaxUnits = 4096; // NEEDLE_REPLACE_MAX_UNITS: the replacement and a chunk's piece table are resident in LDS together
constexpr int kReplaceWaves = 4;            // waves per workgroup; a wave owns a 64-row group at a time
constexpr uint32_t kReplaceChunk = 256;     // matches of a group per piece table
constexpr uint32_t kReplacePutBytes = 2048; // the replacement reaches the device as kernel arguments, this many bytes per launch

struct ReplaceArgs {
    const uint8_t *data;       // the rows' code units (device, 4-byte aligned)
    const uint64_t *in_off;    // n_rows + 1 row offsets, in code units
    uint64_t n_rows;
    uint32_t cw;               // 1 | 2
    uint32_t repl_len;         // code units
    const uint64_t *match_off; // n_rows + 1: row r's matches are start / end[match_off[r] .. match_off[r + 1])
    const int32_t *start, *end;
    const uint8_t *repl;       // fill: repl_len * cw bytes (device, 16-byte aligned, padded to whole 16 bytes)
    uint64_t *out_len;         // lengths: n_rows
    const uint64_t *out_off;   // fill: n_rows + 1, in code units
    uint8_t *out;              // fill: the output code units (device, 4-byte aligned)
};

struct ReplacePiece {
    uint8_t b[kReplacePutBytes];
};

} // namespace needle
