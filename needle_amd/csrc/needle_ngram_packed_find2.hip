// needle_ngram_packed_find2.hip -- the packed-rows filter kernel (needle_ngram_packed.h): OP_FIND, char width 2; and the launcher of all
// four translation units.
#include <stdlib.h>
#include <string.h>
#include "needle_ngram_packed.h"
#include "needle_launch.h"
namespace needle {
hipError_t launch_ngram_packed_contained1(const NgramArgs &A, int n_cus, size_t lds, hipStream_t s);
hipError_t launch_ngram_packed_contained2(const NgramArgs &A, int n_cus, size_t lds, hipStream_t s);
hipError_t launch_ngram_packed_find1(const NgramArgs &A, int n_cus, size_t lds, hipStream_t s);

// LDS a packed launch takes (the program, the bitmaps, per wave the queues, slots and row starts); 0 = does not fit (the caller keeps
// the plain packed kernel)
size_t ngram_packed_lds_bytes(const ProgHeader &h, const NgramParams &ng) {
    NgramLayout l;
    if (ng.addr_shift != 24u) return 0;
    if (ng.on2 && ngram_layout(h.lds_bytes, ng.bm_bytes, &l, kNgWaveLdsPacked, ng.bm2_bytes)) return l.total;
    return ngram_layout(h.lds_bytes, ng.bm_bytes, &l, kNgWaveLdsPacked) ? l.total : 0;
}

// a: rows = the view's data, n_rows, prog / hdr, fixed_len, bitmap, start / end or packed / packed8.  char_width 2 with a byte program:
// the text is narrowed to the pattern's page on load (page, sub: needle_api.cpp utf16_route); ng.wide: hashed as it stands.
hipError_t launch_ngram_packed(int op, const ScanArgs &a, const uint64_t *offsets, int32_t *overflow, const NgramParams &ng, const uint32_t *d_bitmap,
                               uint32_t *d_stats, int n_cus, hipStream_t stream, int char_width, int page, int sub) {
    if (op != OP_FIND && op != OP_CONTAINED_IN) return hipErrorInvalidValue;
    NgramArgs A;
    memset(&A, 0, sizeof(A));
    A.a = a;
    A.ng = ng;
    A.ng_bitmap = d_bitmap;
    A.stats = d_stats;
    A.char_width = (uint32_t)char_width;
    A.page4 = (uint32_t)(page & 255) * 0x01010101u, A.sub4 = (uint32_t)(sub & 255) * 0x01010101u;
    A.stride_log2 = 0xFFFFFFFFu;
    A.pk_offsets = offsets;
    A.pk_overflow = a.packed ? overflow : nullptr;
    // NEEDLE_PACKED_DIRECT_ABOVE (tests): groups whose span exceeds this many chars take the row-by-row walk; never above 2^31 - 1
    static const uint64_t direct_env = getenv("NEEDLE_PACKED_DIRECT_ABOVE") ? (uint64_t)atoll(getenv("NEEDLE_PACKED_DIRECT_ABOVE")) : 0x7FFFFFFFull;
    A.pk_direct_above = direct_env < 0x7FFFFFFFull ? direct_env : 0x7FFFFFFFull;
    if (ng.addr_shift != 24u) return hipErrorInvalidValue;
    if (ng.on2 && !ngram_layout(a.hdr.lds_bytes, ng.bm_bytes, &A.lay, kNgWaveLdsPacked, ng.bm2_bytes)) A.ng.on2 = 0;
    if (!A.ng.on2 && !ngram_layout(a.hdr.lds_bytes, ng.bm_bytes, &A.lay, kNgWaveLdsPacked)) return hipErrorInvalidValue;
    const size_t lds = A.lay.total;
    if (char_width == 2) return op == OP_FIND ? launch_ngp_m<OP_FIND, 2>(A, n_cus, lds, stream) : launch_ngram_packed_contained2(A, n_cus, lds, stream);
    return op == OP_FIND ? launch_ngram_packed_find1(A, n_cus, lds, stream) : launch_ngram_packed_contained1(A, n_cus, lds, stream);
}
} // namespace needle
