// needle_ngram_packed_find_all2.hip -- the packed-rows filter kernel (needle_ngram_packed.h): OP_NG_FIND_ALL, char width 2; and the
// launcher of both find-all translation units.
#include <stdlib.h>
#include <string.h>
#include "needle_ngram_packed.h"
#include "needle_launch.h"
namespace needle {
hipError_t launch_ngram_packed_find_all1(const NgramArgs &A, int n_cus, size_t lds, hipStream_t s);

// LDS a packed find-all launch takes (the program, the bitmaps, per wave the queue(s), the rows' candidate slots and counters and the
// 64 row starts); 0 = does not fit (the caller converts the batch)
size_t ngram_packed_find_all_lds_bytes(const ProgHeader &h, const NgramParams &ng) {
    NgramLayout l;
    if (ng.addr_shift != 24u) return 0;
    if (ng.on2 && ngram_layout(h.lds_bytes, ng.bm_bytes, &l, kNgWaveLdsPackedFA + kNgQueue * 4u, ng.bm2_bytes)) return l.total;
    return ngram_layout(h.lds_bytes, ng.bm_bytes, &l, kNgWaveLdsPackedFA) ? l.total : 0;
}

// Every non-overlapping match of every packed row behind the filter: counting only (counts), or compact filing at the caller's offsets
// (match k of row r at offsets[r] + k, room for offsets[r + 1] - offsets[r]; row-relative int32 starts / ends).  a: rows = the view's data,
// n_rows, prog / hdr, fixed_len.  char_width 2 with a byte program: narrowed to the pattern's page on load; ng.wide: hashed as it stands.
hipError_t launch_ngram_packed_find_all(const ScanArgs &a, const uint64_t *row_offsets, const NgramParams &ng, const uint32_t *d_bitmap, uint32_t *d_stats,
                                        uint32_t *counts, int32_t *starts, int32_t *ends, int32_t *more, const uint64_t *offsets, bool count_only, int n_cus,
                                        hipStream_t stream, int char_width, int page, int sub) {
    if (!more || (count_only ? !counts : (!offsets || !starts || !ends))) return hipErrorInvalidValue;
    NgramArgs A;
    memset(&A, 0, sizeof(A));
    A.a = a;
    A.ng = ng;
    A.ng_bitmap = d_bitmap;
    A.stats = d_stats;
    A.char_width = (uint32_t)char_width;
    A.page4 = (uint32_t)(page & 255) * 0x01010101u, A.sub4 = (uint32_t)(sub & 255) * 0x01010101u;
    A.stride_log2 = 0xFFFFFFFFu;
    A.pk_offsets = row_offsets;
    A.fa_counts = counts, A.fa_starts = starts, A.fa_ends = ends, A.fa_more = more;
    A.fa_offsets = count_only ? nullptr : offsets, A.fa_count_only = count_only ? 1u : 0u;
    // NEEDLE_PACKED_DIRECT_ABOVE (tests): groups whose span exceeds this many chars are searched row by row; never above 2^31 - 1
    static const uint64_t direct_env = getenv("NEEDLE_PACKED_DIRECT_ABOVE") ? (uint64_t)atoll(getenv("NEEDLE_PACKED_DIRECT_ABOVE")) : 0x7FFFFFFFull;
    A.pk_direct_above = direct_env < 0x7FFFFFFFull ? direct_env : 0x7FFFFFFFull;
    if (ng.addr_shift != 24u) return hipErrorInvalidValue;
    // the second level needs its bitmap and a second queue per wave: taken where it still fits (launch_ngram_find_all does the same)
    if (ng.on2 && !ngram_layout(a.hdr.lds_bytes, ng.bm_bytes, &A.lay, kNgWaveLdsPackedFA + kNgQueue * 4u, ng.bm2_bytes)) A.ng.on2 = 0;
    if (!A.ng.on2 && !ngram_layout(a.hdr.lds_bytes, ng.bm_bytes, &A.lay, kNgWaveLdsPackedFA)) return hipErrorInvalidValue;
    const size_t lds = A.lay.total;
    return char_width == 2 ? launch_ngp_m<OP_NG_FIND_ALL, 2>(A, n_cus, lds, stream) : launch_ngram_packed_find_all1(A, n_cus, lds, stream);
}
} // namespace needle
