// Host-side launchers and shape / LDS-footprint queries of the kernels, as needle_api.cpp calls them.  Every file that defines one of them
// includes this header, so a signature or a default argument that drifts apart fails to compile.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <functional>
#include "needle_captures.h"
#include "needle_device.h"
#include "needle_find_all.h"
#include "needle_gather.h"
#include "needle_group.h"
#include "needle_lines.h"
#include "needle_ngram.h"
#include "needle_replace.h"
#include "needle_replace_each.h"
#include "needle_replace_groups.h"

namespace needle {

// needle_kernels.hip: the scan kernels of fixed-stride rows
hipError_t launch_scan(int op, int char_width, const ScanArgs &a, int n_cus, hipStream_t stream);
bool shape_for_program(const ProgHeader &h, int char_width, int *waves, int *chb, int *tiles_in_f_rows);
// needle_packed_find2.hip, needle_packed_find_all2.hip: packed rows scanned where they lie
hipError_t launch_packed(int op, int char_width, const PackedArgs &a, int n_cus, hipStream_t stream);
hipError_t launch_packed_find_all(int char_width, const PackedFindAllArgs &a, int n_cus, hipStream_t stream);
bool packed_find_all_shape(uint32_t prog_lds_bytes, int char_width, int *waves, int *chb);
// needle_packed_find_all_lane2.hip: every match of every packed row for patterns without a transducer (per-lane restarts)
hipError_t launch_packed_find_all_lane(int char_width, const PackedFindAllArgs &a, int n_cus, hipStream_t stream);
bool packed_find_all_lane_mode(uint32_t mode);
bool packed_find_all_lane_shape(uint32_t prog_lds_bytes, int char_width, int *waves, int *chb);
// needle_packed_set2.hip: a pattern set's group on packed rows (needle_packed_set.h); op: OP_MATCHES | OP_CONTAINED_IN
hipError_t launch_packed_set(int op, int char_width, const PackedSetArgs &a, int n_cus, hipStream_t stream);
// needle_set_spans2.hip: a pattern set's group on a CSR span list of packed rows (needle_set_spans.h): which members match each span
hipError_t launch_set_spans(int char_width, const SetSpansArgs &a, int n_cus, hipStream_t stream);
// needle_captures_spans2.hip: the capturing groups of each span of a CSR span list of packed rows (needle_captures_spans.h)
hipError_t launch_captures_spans(int char_width, const CapSpansArgs &a, int n_cus, hipStream_t stream);
// needle_compact.hip
int compact_blocked16(uint64_t n, uint32_t max_per_row, uint64_t *d_offsets, uint32_t *d_start_end16, uint64_t cap, uint64_t *d_total, hipStream_t stream,
                      const std::function<int(uint32_t *counts, uint32_t *blocks)> &fill);
// needle_find_all.hip, needle_find_all_ls.hip: every match of every row in one pass
hipError_t launch_find_all(int char_width, const FindAllArgs &fa, int n_cus, hipStream_t stream);
bool find_all_lane_shape(uint32_t prog_lds_bytes, int *waves, int *chb); // (the per-lane kernels' one candidate list, packed rows included)
hipError_t launch_find_all_lockstep(int char_width, const FindAllArgs &fa, int n_cus, hipStream_t stream);
bool find_all_lockstep_shape_ok(const FindAllArgs &fa);
// (the lock-step kernels' one candidate list and launch geometry, packed rows included; tiles128: 128-byte tiles per lane allowed)
bool find_all_lockstep_shape(uint32_t prog_lds_bytes, bool tiles128, int *waves, int *chb);
void find_all_lockstep_grid(uint32_t prog_lds_bytes, uint64_t n_rows, int waves, int chb, int n_cus, int *grid, size_t *lds);
// needle_stripe.hip: few long rows (stripes, speculative stripes), the round-per-match find-all's collect pass, packed -> fixed stride
hipError_t launch_find_all_collect(uint64_t n_rows, uint32_t slots, uint32_t k, const int32_t *s, const int32_t *e, int32_t *cursor,
                                   uint32_t *counts, int32_t *starts, int32_t *ends, int32_t *any_hit, int n_cus, hipStream_t stream);
hipError_t launch_long_rows(int char_width, const StripeArgs &a, int n_cus, hipStream_t stream);
hipError_t launch_spec_len(const SpecArgs &a, hipStream_t stream);
hipError_t launch_spec_init(const SpecArgs &a, hipStream_t stream);
hipError_t launch_spec_fix(const SpecArgs &a, hipStream_t stream);
hipError_t launch_spec_reduce(const SpecArgs &a, hipStream_t stream);
hipError_t launch_backward_rows(int char_width, const StripeArgs &a, hipStream_t stream);
hipError_t launch_unpack(const void *data, const uint64_t *offsets, uint64_t n_rows, uint32_t cw, void *out,
                         uint64_t stride_bytes, uint32_t *lengths, int32_t *overflow, int n_cus, hipStream_t stream);
#ifdef NEEDLE_TUNING // needle_dict.hip (two row sets per wave; measured, no faster -- DESIGN.md s4) is part of measurement builds only
bool dict_kernel_applies(int char_width, const ScanArgs &a);
hipError_t launch_dict(int op, const ScanArgs &a, int n_cus, hipStream_t stream);
#endif
// needle_ngram.hip: containedIn / find behind the n-gram candidate filter
bool ngram_shape_ok(const ScanArgs &a);
size_t ngram_lds_bytes(const ProgHeader &h, const NgramParams &ng);
hipError_t launch_ngram(int op, const ScanArgs &a, const NgramParams &ng, const uint32_t *d_bitmap, uint32_t *d_stats, int n_cus, hipStream_t stream,
                        int char_width = 1, int page = 0, int sub = 0xFF);
size_t ngram_find_all_lds_bytes(const ProgHeader &h, const NgramParams &ng);
hipError_t launch_ngram_find_all(const ScanArgs &a, const NgramParams &ng, const uint32_t *d_bitmap, uint32_t *d_stats, uint32_t slots, uint32_t *counts,
                                 int32_t *starts, int32_t *ends, uint32_t *packed, int32_t *more, const uint64_t *offsets, bool count_only, int n_cus,
                                 hipStream_t stream, int char_width, int page, int sub, uint32_t kshift);
// needle_ngram_packed_find2.hip: the same filter in front of packed rows (needle_ngram_packed.h)
size_t ngram_packed_lds_bytes(const ProgHeader &h, const NgramParams &ng);
hipError_t launch_ngram_packed(int op, const ScanArgs &a, const uint64_t *offsets, int32_t *overflow, const NgramParams &ng, const uint32_t *d_bitmap,
                               uint32_t *d_stats, int n_cus, hipStream_t stream, int char_width, int page, int sub);
// needle_ngram_packed_find_all2.hip: ... and its find-all form (counting, or compact filing at the caller's offsets)
size_t ngram_packed_find_all_lds_bytes(const ProgHeader &h, const NgramParams &ng);
hipError_t launch_ngram_packed_find_all(const ScanArgs &a, const uint64_t *row_offsets, const NgramParams &ng, const uint32_t *d_bitmap, uint32_t *d_stats,
                                        uint32_t *counts, int32_t *starts, int32_t *ends, int32_t *more, const uint64_t *offsets, bool count_only, int n_cus,
                                        hipStream_t stream, int char_width, int page, int sub);
// needle_replace.hip: the splice of needle_replace_all_*_packed_dev (lengths, fill) and the replacement's way to the device
hipError_t launch_replace_put(const void *repl_host, uint32_t bytes, uint8_t *d_repl, hipStream_t stream);
hipError_t launch_replace_lengths(const ReplaceArgs &a, int n_cus, hipStream_t stream);
hipError_t launch_replace_fill(const ReplaceArgs &a, int n_cus, hipStream_t stream);
// needle_replace_each.hip: the splice with a replacement per match out of a table (needle_replace_each_*_packed_dev)
hipError_t launch_replace_each_lengths(const ReplaceEachArgs &a, int n_cus, hipStream_t stream);
hipError_t launch_replace_each_fill(const ReplaceEachArgs &a, int n_cus, hipStream_t stream);
// needle_replace_groups.hip: the splice with a template of literals and group references (needle_replace_groups_*_packed_dev)
hipError_t launch_replace_groups_lengths(const ReplaceGroupsArgs &a, int n_cus, hipStream_t stream);
hipError_t launch_replace_groups_fill(const ReplaceGroupsArgs &a, int n_cus, hipStream_t stream);
// needle_gather.hip: spans of packed rows as a new packed batch (needle_gather_spans_*_packed_dev), a match list's complement
// (needle_split_spans_packed_dev); the spans the fill kernel tables at once
hipError_t launch_gather_lengths(const GatherArgs &a, int n_cus, hipStream_t stream);
hipError_t launch_gather_fill(const GatherArgs &a, int n_cus, hipStream_t stream);
hipError_t launch_split_spans(const GatherArgs &a, int n_cus, hipStream_t stream);
uint32_t gather_chunk_spans();
// needle_group.hip: equal spans of a CSR list put into groups (needle_group_spans_packed_dev): hash, insert, finish on one stream
hipError_t launch_group_spans(const GroupArgs &a, int n_cus, hipStream_t stream);
// needle_utf8.hip: UTF-8 packed rows -> UTF-16 packed rows (lengths, fill), unit positions -> byte offsets; the text a wave takes per step
hipError_t launch_utf8_lengths(const Utf8Args &a, int n_cus, hipStream_t stream);
hipError_t launch_utf8_fill(const Utf8Args &a, int n_cus, hipStream_t stream);
hipError_t launch_utf8_positions(const Utf8Args &a, int n_cus, hipStream_t stream);
uint32_t utf8_window_bytes();
// needle_lines.hip: packed documents cut at their line terminators (needle_lines_*_packed_dev); the units of a tile per char width
hipError_t launch_lines_count(const LinesArgs &a, int n_cus, hipStream_t stream);
hipError_t launch_lines_fill(const LinesArgs &a, bool keep_ends, int n_cus, hipStream_t stream);
uint32_t lines_tile_units(uint32_t char_width);
// needle_lower.cpp (NEEDLE_PREFILTER)
int ngram_level();

} // namespace needle
