// needle_lines.h -- what needle_lines.hip's two kernels (needle_lines_count_packed_dev / needle_lines_fill_packed_dev) take: a packed batch of
// DOCUMENTS (files, multi-line cells) to be cut at their line terminators into a packed batch of LINES.  Pure functions of the text: no
// pattern.
//
// Unlike every other packed kernel, the unit of work is not a 64-row group but a TILE: kLinesTileBytes of `data` at a fixed place, whatever
// documents lie there.  One document of a gigabyte is 10^5 tiles; rows are never walked by a lane.
#pragma once
#include <stdint.h>

namespace needle {

constexpr int kLinesLanes = 256;                // lanes per workgroup; a workgroup owns a tile at a time
constexpr uint32_t kLinesBlocksPerLane = 2;     // aligned 16-byte blocks of a tile per lane
constexpr uint32_t kLinesTileBytes = kLinesLanes * kLinesBlocksPerLane * 16u; // 8192: T = 8192 units at char width 1, 4096 at 2

struct LinesArgs {
    const uint8_t *data;       // the documents' code units (device, 4-byte aligned)
    const uint64_t *in_off;    // n_rows + 1 document offsets, in code units
    uint64_t n_rows;
    uint32_t cw;               // 1 | 2
    uint64_t data_units;       // the caller's upper bound of in_off[n_rows]: fixes the number of tiles
    uint64_t tiles;            // ceil(data_units / T)
    uint64_t *tile_lines;      // count: events per tile
    uint64_t *tile_units;      // count: kept units per tile (STRIP; may be NULL)
    const uint64_t *line_base; // fill: tiles + 1, the exclusive prefix sum of tile_lines
    const uint64_t *unit_base; // fill, STRIP: tiles + 1, the exclusive prefix sum of tile_units
    uint64_t *out_off;         // fill: line j ends at out_off[j + 1]
    uint8_t *out;              // fill, STRIP: the lines' code units (device, 4-byte aligned)
    uint64_t *doc_lines;       // fill: optional, n_rows + 1: the lines in front of each document
};

} // namespace needle
